"""pq_dba_lengths + pq_dba_expand (ops/csrc/parquet_delta_bytearray.hip) on
synthetic DELTA_BYTE_ARRAY pages: well-formed pages against plain `bytes`
concatenation, malformed ones against the status they must get. The output
has guard bytes on both sides and starts at an odd address."""
import numpy as np
import pytest
import torch

import pq_encode as E

MAXV = 4096       # kMaxValue
GUARD = 37
FILL_OUT = 0xEE


def _front_code(values, share=True):
    """(prefix lengths, suffixes) of `values`; share=False codes every value
    whole (p = 0), which the format allows."""
    pre, suf, prev = [], [], b""
    for v in values:
        k = 0
        while share and k < min(len(prev), len(v)) and prev[k] == v[k]:
            k += 1
        pre.append(k)
        suf.append(v[k:])
        prev = v
    return pre, suf


def _page(pre, suf, suf_lens=None, cut=0):
    lens = [len(s) for s in suf] if suf_lens is None else suf_lens
    body = b"".join(suf)
    return (E.delta_binary_packed(pre)[0] + E.delta_binary_packed(lens)[0]
            + body[:len(body) - cut])


def _sorted_keys(rng, n, width=12):
    return sorted(b"key/%0*d" % (width, int(x)) for x in rng.integers(0, 10**9, n))


def _cases():
    rng = np.random.default_rng(7)
    pfx = bytes(rng.integers(0, 256, 40, dtype=np.uint8))
    big = bytes(rng.integers(0, 256, MAXV, dtype=np.uint8))
    ladder = [b"abcdefghijklmnop"[:k] + bytes([200 + i]) for i, k in
              enumerate([16, 12, 8, 3, 0, 1, 5, 9, 16, 16, 2, 15])]
    c = {
        "batch_edges": [_sorted_keys(rng, n) for n in (0, 1, 63, 64, 65, 130)],
        "one_page": [_sorted_keys(rng, 130)],
        "four_pages": [_sorted_keys(rng, 70) for _ in range(4)],
        "five_pages": [_sorted_keys(rng, 70) for _ in range(5)],
        "repeats": [[b"same value, 23 bytes.."] * 150],
        "empties": [[b"", b"", b"ab", b"", b"", b"abc", b"abd", b""] * 20],
        "carried_prefix": [[pfx + bytes([i % 2, i % 251]) for i in range(200)]],
        "shrink_grow": [ladder * 12],
        # ~1 KiB suffixes from a skewed start: they straddle every edge of the 4 KiB window
        "window_edges": [[bytes([i]) + rng.bytes(900 + 37 * i) for i in range(24)]],
        "max_value": [[big, big, big[:-1] + b"\x00", big[:4000] + big[:96], b"", big]],
        "binary": [[rng.bytes(int(k)) for k in rng.integers(0, 40, 300)]],
    }
    cases = [pytest.param(pages, True, id=name) for name, pages in c.items()]
    cases.append(pytest.param(c["four_pages"], False, id="all_p0"))
    return cases


def _launch(payloads, counts, dev="cuda:0"):
    """Lay the pages out at all four skews, decode them, and return
    (status, lengths, value bytes) after checking the guards."""
    from sail_amd.ops import kernels

    ext = kernels.require()
    lay = E.Layout()
    rows, row = [], 0
    for i, (pl, n) in enumerate(zip(payloads, counts)):
        rows.append((lay.add(pl, skew=(i + 1) % 4), len(pl), n, row, 0, 0))
        row += n
    buf, table = lay.finish().to(dev), E.page_table(rows).to(dev)
    prefix, suffix, lengths, sstart, status = ext.pq_dba_lengths(buf, table, row)
    offsets = torch.full((row + 1,), GUARD, dtype=torch.int64, device=dev)
    offsets[1:] += torch.cumsum(lengths, 0)
    total = int(offsets[-1].item()) - GUARD
    out = torch.full((total + 2 * GUARD,), FILL_OUT, dtype=torch.uint8, device=dev)
    ext.pq_dba_expand(buf, table, prefix, suffix, sstart, offsets, lengths,
                      status, out)
    torch.cuda.synchronize()
    raw = out.cpu().numpy().tobytes()
    assert raw[:GUARD] == raw[GUARD + total:] == bytes([FILL_OUT]) * GUARD
    return status.cpu().tolist(), lengths.cpu().tolist(), raw[GUARD:GUARD + total]


@pytest.mark.gpu
@pytest.mark.parametrize("pages,share", _cases())
def test_pages_decode_to_their_values(pages, share):
    payloads = [_page(*_front_code(vals, share)) for vals in pages]
    status, lengths, blob = _launch(payloads, [len(v) for v in pages])
    flat = [v for vals in pages for v in vals]
    assert status == [0] * len(pages)
    assert lengths == [len(v) for v in flat]
    assert blob == b"".join(flat)


_BAD = {
    # name: (page bytes, n_values, status)
    "first_prefix_not_zero": (_page([1, 0], [b"ab", b"cd"]), 2, 4),
    "prefix_longer_than_previous": (_page([0, 5], [b"abc", b"d"]), 2, 4),
    "negative_suffix_length": (_page([0, 0, 0], [b"abc", b"de"], [3, -1, 2]), 3, 2),
    "suffix_bytes_cut_short": (_page([0, 1], [b"abc", b"def"], cut=2), 2, 6),
    "value_too_long": (_page([0, 0], [b"x", b"y" * (MAXV + 1)]), 2, 5),
    "more_values_than_rows": (_page([0] * 5, [b"v"] * 5), 3, 8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_BAD))
def test_malformed_page_is_refused_by_status(name):
    bad, n, want = _BAD[name]
    good = _sorted_keys(np.random.default_rng(3), 70)
    ok = _page(*_front_code(good))
    status, lengths, blob = _launch([ok, bad, ok], [70, n, 70])
    assert status == [0, want, 0]
    assert lengths == [len(v) for v in good] + [0] * n + [len(v) for v in good]
    assert blob == b"".join(good) * 2
