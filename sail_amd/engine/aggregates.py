"""Group-by aggregation (torch path).

Reference implementation of the ~sail-function aggregate surface
(ref: crates/sail-function/src/aggregate/) over dense group ids; the GPU hot
path is the HIP hash-aggregate kernel (ops/csrc/hash_agg.hip) validated
against this module.
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch

from . import types as T
from .column import Column, StringColumn
from .joins import normalize_key


def group_ids(keys: List[Column], mask: Optional[torch.Tensor] = None
              ) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Returns (gid per row, representative row index per group, n_groups).
    Null keys form their own groups (SQL GROUP BY semantics).

    `mask`: optional selection — groups are defined by masked-in rows only
    (masked-out rows get an arbitrary gid the caller must also mask).

    Fast path: when the combined key domain is dense (dict codes, dense
    surrogate keys like l_orderkey) the gids come from a presence-bitmap +
    prefix-sum remap — no sort. The torch.unique sort path only runs for
    genuinely sparse domains (e.g. hashed raw strings)."""
    if not keys:
        raise ValueError("group_ids requires keys")
    dev = keys[0].device
    n = len(keys[0])
    norm = []
    from .column import StringColumn as _SC
    from .joins import exact_string_codes

    raw_str = [i for i, c in enumerate(keys)
               if isinstance(c, _SC) and not c.is_dict]
    exact = {}
    if raw_str:
        # raw-string keys: exact dense codes (128-bit hash + byte-verify),
        # not FNV-64 — grouping must never merge distinct strings
        codes = exact_string_codes([keys[i] for i in raw_str])
        exact = dict(zip(raw_str, codes))
    for i, c in enumerate(keys):
        k = exact[i] if i in exact else normalize_key(c)
        if c.validity is not None:
            # give nulls a dedicated code below the domain
            k = torch.where(c.valid_mask(), k, torch.full_like(k, k.min().item() - 1 if n else -1))
        norm.append(k)

    # dense-domain fast path
    if n > 0:
        mins, spans = [], []
        total = 1
        for k in norm:
            lo = int(k.min().item())
            hi = int(k.max().item())
            mins.append(lo)
            spans.append(hi - lo + 1)
            total *= spans[-1]
            if total > max(4 * n, 1 << 22) or total > (1 << 31):
                total = -1
                break
        if total > 0:
            packed = norm[0] - mins[0]
            for i in range(1, len(norm)):
                packed = packed * spans[i] + (norm[i] - mins[i])
            present = torch.zeros(total, dtype=torch.bool, device=dev)
            sel = packed if mask is None else packed[mask]
            present[sel] = True
            lut = torch.cumsum(present.to(torch.int32), 0) - 1
            gid = lut.index_select(0, packed).to(torch.int64)
            ng = int(present.sum().item())
            rep = _any_representative(gid, n, ng, mask, dev)
            return gid, rep, ng

    if n == 0:
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        return empty, empty, 0
    # sparse domain: reduce multi-key to ONE int64 — exact range packing when
    # the combined span fits, otherwise a mixed 64-bit hash combine (collision
    # odds ~n^2/2^64; documented engine tradeoff, exact for <=2 keys in range)
    if len(norm) > 1:
        packed1 = _pack_or_hash(norm)
    else:
        packed1 = norm[0]
    # NOTE: a sort-free hash group-id kernel exists (hg_group in
    # ops/csrc/hash_join.hip, validated by tests/test_gpu.py) but measured
    # SLOWER than this unique-sort path end-to-end (ClickBench 1.19s ->
    # 1.33s): rocPRIM onesweep sorts at ~3 GB/ms beat random-scatter CAS
    # claims + table gathers at these shapes, so the sort path stays.
    if mask is None:
        # unique's inverse IS the gid — recomputing it with searchsorted
        # cost ~20 ms per 100M-row call (ClickBench q32 profile)
        uniq, gid = torch.unique(packed1, return_inverse=True)
        ng = int(uniq.shape[0])
        rep = _any_representative(gid, n, ng, None, dev)
        return gid, rep, ng
    sel = packed1[mask]
    uniq = torch.unique(sel)
    gid = torch.searchsorted(uniq, packed1).clamp(0, max(uniq.shape[0] - 1, 0))
    ng = int(uniq.shape[0])
    rep = _any_representative(gid, n, ng, mask, dev)
    return gid, rep, ng


def _pack_or_hash(norm: List[torch.Tensor]) -> torch.Tensor:
    """Combine multiple int64 key columns into one: exact range packing when
    the span product fits int64, else a murmur-style mixed hash combine."""
    mins, spans = [], []
    total = 1
    ok = True
    for k in norm:
        lo = int(k.min().item())
        hi = int(k.max().item())
        mins.append(lo)
        spans.append(hi - lo + 1)
        total *= spans[-1]
        if total > (1 << 62):
            ok = False
            break
    if ok:
        acc = norm[0] - mins[0]
        for i in range(1, len(norm)):
            acc = acc * spans[i] + (norm[i] - mins[i])
        return acc
    acc = norm[0].clone()
    for i in range(1, len(norm)):
        acc = acc * 31 + norm[i]
        mixed = acc ^ (acc >> 33)
        mixed = mixed * -49064778989728563  # 0xFF51AFD7ED558CCD signed
        acc = mixed ^ (mixed >> 33)
    return acc


def _any_representative(gid, n, ng, mask, dev):
    """ANY row index per group (rows in a group share identical key values,
    so key-gathering doesn't need the first occurrence). Plain scatter assign
    is ~1000x faster than scatter_reduce(amin) on ROCm."""
    rep = torch.zeros(ng, dtype=torch.int64, device=dev)
    rows = torch.arange(n, device=dev)
    if mask is None:
        rep.scatter_(0, gid, rows)
    else:
        rep.scatter_(0, gid[mask], rows[mask])
    return rep


class MaskedGroupsUnsupported(Exception):
    """group_ids(mask=...) fallback signal for sparse multi-key domains."""


def _masked(values: Column, extra_mask: Optional[torch.Tensor]):
    mask = values.valid_mask()
    if extra_mask is not None:
        mask = mask & extra_mask
    return mask


#: user-defined aggregates: name -> (fn(list_of_group_values) -> scalar, type)
#: engine-wide (registered via session.udf.register_aggregate); evaluated on
#: host per group — the pyo3 UDAF boundary of the reference
#: (ref: crates/sail-python-udf aggregate UDFs) as an in-process call.
UDAFS: dict = {}


def _udaf_eval(name, args, gid, ng, filter_mask, out_type):
    fn, rt = UDAFS[name]
    rt = out_type or rt
    c = args[0]
    mask = _masked(c, filter_mask)
    gl = gid[mask].cpu().tolist()
    import torch as _t

    kept = _t.nonzero(mask, as_tuple=False).flatten()
    if len(args) > 1:  # multi-arg UDAF (e.g. tuple_sketch_agg(key, value))
        per_arg = [a.gather(kept.to(a.device)).to_pylist() for a in args]
        vals = list(zip(*per_arg))
    else:
        vals = c.gather(kept.to(c.device)).to_pylist()
    groups = [[] for _ in range(ng)]
    for g, v in zip(gl, vals):
        groups[g].append(v)
    out = [fn(gvals) for gvals in groups]
    return Column.from_values(out, rt, device=gid.device)


def agg_eval(name: str, args: List[Column], gid: torch.Tensor, ng: int,
             distinct: bool = False, filter_mask: Optional[torch.Tensor] = None,
             out_type: T.DataType = None) -> Column:
    """Evaluate one aggregate over groups. args already evaluated per-row."""
    dev = gid.device
    if name.endswith("_agg") and name not in UDAFS:
        from . import functions_impl  # noqa: F401  (registers sketch UDAFS)
    if name in UDAFS:
        return _udaf_eval(name, args, gid, ng, filter_mask, out_type)
    if name == "count" and not args:
        mask = filter_mask if filter_mask is not None else torch.ones(gid.shape[0], dtype=torch.bool, device=dev)
        data = torch.zeros(ng, dtype=torch.int64, device=dev)
        data.index_add_(0, gid[mask], torch.ones(int(mask.sum()), dtype=torch.int64, device=dev))
        return Column(T.I64, data, None)

    c = args[0]
    mask = _masked(c, filter_mask)
    if distinct and name in ("count", "sum", "avg"):
        ext = _distinct_ext(name, c, gid, ng)
        if ext is not None:
            return _distinct_finish(name, _distinct_hash(ext, c, gid, ng, mask, name != "count"),
                                    c, out_type)
        _took_distinct("sort")
        # unique (gid, value) pairs via two stable sorts — torch.unique(dim=0)
        # has an allocation-state-dependent crash on ROCm at ~1e8 rows
        vk = normalize_key(c)
        gm, vm = gid[mask], vk[mask]
        if gm.numel():
            ord1 = torch.argsort(vm)
            g1 = gm.index_select(0, ord1)
            ord2 = torch.argsort(g1, stable=True)
            g_sorted = g1.index_select(0, ord2)
            v_sorted = vm.index_select(0, ord1).index_select(0, ord2)
            first = torch.ones(g_sorted.shape[0], dtype=torch.bool, device=dev)
            first[1:] = (g_sorted[1:] != g_sorted[:-1]) | (v_sorted[1:] != v_sorted[:-1])
            ugid = g_sorted[first]
            uvals = v_sorted[first]
        else:
            ugid = torch.zeros(0, dtype=torch.int64, device=dev)
            uvals = torch.zeros(0, dtype=torch.int64, device=dev)
        if name == "count":
            data = torch.zeros(ng, dtype=torch.int64, device=dev)
            data.index_add_(0, ugid, torch.ones(ugid.shape[0], dtype=torch.int64, device=dev))
            return Column(T.I64, data, None)
        # sum/avg distinct: normalized keys ARE the raw values for int-like
        vals = uvals
        data = torch.zeros(ng, dtype=torch.int64, device=dev)
        data.index_add_(0, ugid, vals)
        if name == "avg":
            cnt = torch.zeros(ng, dtype=torch.int64, device=dev)
            cnt.index_add_(0, ugid, torch.ones(ugid.shape[0], dtype=torch.int64, device=dev))
            return _avg_result(data, cnt, c.dtype, out_type)
        return Column(out_type or T.I64, data, None)

    if name in ("collect_list", "array_agg", "collect_set"):
        from .column import ListColumn

        m = mask & c.valid_mask()  # Spark: nulls are dropped from collections
        gm = gid[m]
        kept = torch.nonzero(m, as_tuple=False).flatten()
        if name == "collect_set":
            vk = normalize_key(c)[m]
            o1 = torch.argsort(vk, stable=True)
            o2 = torch.argsort(gm.index_select(0, o1), stable=True)
            order = o1.index_select(0, o2)
            gs = gm.index_select(0, order)
            vs = vk.index_select(0, order)
            first = torch.ones(gs.shape[0], dtype=torch.bool, device=dev)
            if gs.shape[0] > 1:
                first[1:] = (gs[1:] != gs[:-1]) | (vs[1:] != vs[:-1])
            kept = kept.index_select(0, order)[first]
            gm = gs[first]
        else:
            order = torch.argsort(gm, stable=True)
            kept = kept.index_select(0, order)
            gm = gm.index_select(0, order)
        lens = torch.bincount(gm, minlength=ng)
        offs = torch.zeros(ng + 1, dtype=torch.int64, device=dev)
        torch.cumsum(lens, 0, out=offs[1:])
        return ListColumn(offs, c.gather(kept))

    if name in ("median", "percentile", "percentile_approx", "percentile_disc"):
        out = _percentile_device(name, args, c, gid, ng, mask)
        if out is not None:
            return out
        _took_percentile("host")

    gidm = gid[mask]
    n_used = int(mask.sum().item())

    if name == "count":
        data = torch.zeros(ng, dtype=torch.int64, device=dev)
        data.index_add_(0, gidm, torch.ones(n_used, dtype=torch.int64, device=dev))
        return Column(T.I64, data, None)

    if name == "sumf":
        vals = c.data[mask].to(torch.float64)
        if isinstance(c.dtype, T.DecimalType):
            vals = vals / (10.0 ** c.dtype.scale)
        data = torch.zeros(ng, dtype=torch.float64, device=dev)
        data.index_add_(0, gidm, vals)
        return Column(T.F64, data, None)

    if name == "sumsq":
        vals = c.data[mask].to(torch.float64)
        if isinstance(c.dtype, T.DecimalType):
            vals = vals / (10.0 ** c.dtype.scale)
        data = torch.zeros(ng, dtype=torch.float64, device=dev)
        data.index_add_(0, gidm, vals * vals)
        return Column(T.F64, data, None)

    if name == "count_if":
        vals = c.data[mask].to(torch.int64)
        data = torch.zeros(ng, dtype=torch.int64, device=dev)
        data.index_add_(0, gidm, vals)
        return Column(T.I64, data, None)

    if name in ("sum", "try_sum"):
        if isinstance(c.dtype, T.DecimalType) or c.dtype.is_integer:
            vals = c.data[mask].to(torch.int64)
            acc_t = torch.int64
        else:
            vals = c.data[mask].to(torch.float64)
            acc_t = torch.float64
        data = torch.zeros(ng, dtype=acc_t, device=dev)
        data.index_add_(0, gidm, vals)
        cnt = torch.zeros(ng, dtype=torch.int64, device=dev)
        cnt.index_add_(0, gidm, torch.ones(n_used, dtype=torch.int64, device=dev))
        validity = (cnt > 0).to(torch.uint8)
        rt = out_type or (T.DecimalType(38, c.dtype.scale) if isinstance(c.dtype, T.DecimalType)
                          else (T.I64 if c.dtype.is_integer else T.F64))
        if isinstance(rt, T.DecimalType) and isinstance(c.dtype, T.DecimalType) and rt.scale != c.dtype.scale:
            from .eval import _rescale_int

            data = _rescale_int(data, c.dtype.scale, rt.scale)
        return Column(rt, data, None if bool((cnt > 0).all()) else validity)

    if name in ("avg", "try_avg"):
        if isinstance(c.dtype, T.DecimalType) or c.dtype.is_integer:
            vals = c.data[mask].to(torch.int64)
            data = torch.zeros(ng, dtype=torch.int64, device=dev)
        else:
            vals = c.data[mask].to(torch.float64)
            data = torch.zeros(ng, dtype=torch.float64, device=dev)
        data.index_add_(0, gidm, vals)
        cnt = torch.zeros(ng, dtype=torch.int64, device=dev)
        cnt.index_add_(0, gidm, torch.ones(n_used, dtype=torch.int64, device=dev))
        return _avg_result(data, cnt, c.dtype, out_type)

    if name in ("min", "max"):
        red = "amin" if name == "min" else "amax"
        if isinstance(c, StringColumn):
            # order by dict code only if dictionary is sorted; our dictionaries
            # are built sorted (column.py from_pylist), so codes order == value order
            vals = normalize_key(c)[mask]
            data = torch.full((ng,), 2**62 if name == "min" else -(2**62), dtype=torch.int64, device=dev)
            data.scatter_reduce_(0, gidm, vals, reduce=red, include_self=True)
            cnt = torch.zeros(ng, dtype=torch.int64, device=dev)
            cnt.index_add_(0, gidm, torch.ones(n_used, dtype=torch.int64, device=dev))
            if c.is_dict:
                return StringColumn(c.offsets, c.bytes_,
                                    None if bool((cnt > 0).all()) else (cnt > 0).to(torch.uint8),
                                    data.to(torch.int32))
            # raw strings: order-preserving dense ranks, then pick the row
            # holding the group's best rank and gather the actual string
            from .executor import _sortable

            ranks = _sortable(c)
            big = int(ranks.max().item()) + 1 if ranks.numel() else 1
            rv = torch.where(mask, ranks, torch.full_like(ranks, big if name == "min" else -1))
            best = torch.full((ng,), big if name == "min" else -1,
                              dtype=torch.int64, device=dev)
            best.scatter_reduce_(0, gid, rv, reduce=red, include_self=True)
            is_best = (rv == best[gid]) & mask
            rows = torch.full((ng,), 0, dtype=torch.int64, device=dev)
            rows.scatter_(0, gid[is_best], torch.arange(gid.shape[0], device=dev)[is_best])
            got = c.gather(rows)
            valid = cnt > 0
            got.validity = None if bool(valid.all()) else valid.to(torch.uint8)
            return got
        vals = c.data[mask]
        if vals.dtype.is_floating_point:
            init = float("inf") if name == "min" else float("-inf")
        else:
            info = torch.iinfo(vals.dtype)
            init = info.max if name == "min" else info.min
        data = torch.full((ng,), init, dtype=vals.dtype, device=dev)
        data.scatter_reduce_(0, gidm, vals, reduce=red, include_self=True)
        cnt = torch.zeros(ng, dtype=torch.int64, device=dev)
        cnt.index_add_(0, gidm, torch.ones(n_used, dtype=torch.int64, device=dev))
        return Column(out_type or c.dtype, data,
                      None if bool((cnt > 0).all()) else (cnt > 0).to(torch.uint8))

    if name in ("first", "last", "any_value"):
        sel = torch.arange(gid.shape[0], device=dev)[mask]
        init = gid.shape[0] if name != "last" else -1
        red = "amin" if name != "last" else "amax"
        rep = torch.full((ng,), init, dtype=torch.int64, device=dev)
        rep.scatter_reduce_(0, gidm, sel, reduce=red, include_self=True)
        ok = rep != init
        safe = torch.where(ok, rep, torch.zeros_like(rep))
        res = c.gather(safe)
        if not bool(ok.all()):
            v = res.valid_mask() & ok
            if isinstance(res, StringColumn):
                res.validity = v.to(torch.uint8)
            else:
                res = Column(res.dtype, res.data, v.to(torch.uint8))
        return res

    if name in ("stddev_samp", "stddev_pop", "var_samp", "var_pop"):
        vals = c.data[mask].to(torch.float64)
        if isinstance(c.dtype, T.DecimalType):
            vals = vals / (10.0 ** c.dtype.scale)
        s1 = torch.zeros(ng, dtype=torch.float64, device=dev)
        s2 = torch.zeros(ng, dtype=torch.float64, device=dev)
        cnt = torch.zeros(ng, dtype=torch.float64, device=dev)
        s1.index_add_(0, gidm, vals)
        s2.index_add_(0, gidm, vals * vals)
        cnt.index_add_(0, gidm, torch.ones(n_used, dtype=torch.float64, device=dev))
        mean = s1 / cnt.clamp_min(1)
        m2 = s2 - cnt * mean * mean
        denom = cnt - (1.0 if name.endswith("_samp") else 0.0)
        var = m2 / denom.clamp_min(1e-300)
        var = var.clamp_min(0)
        data = torch.sqrt(var) if name.startswith("stddev") else var
        valid = denom > 0
        return Column(T.F64, data, None if bool(valid.all()) else valid.to(torch.uint8))

    if name in ("any", "bool_and"):
        vals = c.data[mask].to(torch.bool)
        if name == "any":
            data = torch.zeros(ng, dtype=torch.bool, device=dev)
            data.scatter_reduce_(0, gidm, vals, reduce="amax", include_self=True)
        else:
            data = torch.ones(ng, dtype=torch.bool, device=dev)
            data.scatter_reduce_(0, gidm, vals, reduce="amin", include_self=True)
        return Column(T.BOOL, data, None)

    if name == "product":
        vals = c.data[mask].to(torch.float64)
        data = torch.ones(ng, dtype=torch.float64, device=dev)
        data.scatter_reduce_(0, gidm, vals, reduce="prod", include_self=True)
        return Column(T.F64, data, None)

    if name == "percentile_disc":
        # discrete percentile: smallest value with cdf >= q; row-gather
        # preserves the input dtype exactly
        import math as _math

        q = float(args[1].to_pylist()[0]) if len(args) > 1 and len(args[1]) else 0.5
        desc = bool(args[2].to_pylist()[0]) if len(args) > 2 and len(args[2]) else False
        ridx = torch.nonzero(mask, as_tuple=False).flatten()
        vals = c.data[mask].to(torch.float64)
        g = gid[mask]
        import collections

        groups = collections.defaultdict(list)
        for rr, gg, vv in zip(ridx.tolist(), g.tolist(), vals.tolist()):
            groups[gg].append((vv, rr))
        pick = torch.zeros(ng, dtype=torch.int64, device=dev)
        has = torch.zeros(ng, dtype=torch.bool, device=dev)
        for k, lst in groups.items():
            lst.sort(reverse=desc)
            n_ = len(lst)
            i = max(0, min(n_ - 1, _math.ceil(q * n_) - 1))
            pick[k] = lst[i][1]
            has[k] = True
        out = c.gather(pick)
        if not bool(has.all()):
            v = out.valid_mask() & has
            out = Column(out.dtype, out.data, v.to(torch.uint8)) \
                if not isinstance(out, StringColumn) else out
        return out

    if name in ("vector_sum", "vector_avg"):
        from .column import ListColumn

        lens = c.lengths()
        rows_mask = mask
        L = int(lens[rows_mask].max().item()) if bool(rows_mask.any()) else 0
        seg = c.segment_ids()
        emask = rows_mask[seg]
        pos = torch.arange(seg.shape[0], dtype=torch.int64, device=dev) \
            - c.offsets[:-1][seg]
        tgt = gid[seg] * L + pos
        out = torch.zeros(ng * L, dtype=torch.float64, device=dev)
        out.index_add_(0, tgt[emask],
                       c.child.data.to(torch.float64)[emask])
        if name == "vector_avg":
            cnt = torch.zeros(ng, dtype=torch.float64, device=dev)
            cnt.index_add_(0, gid[rows_mask],
                           torch.ones(int(rows_mask.sum()),
                                      dtype=torch.float64, device=dev))
            out = out / cnt.clamp_min(1.0).repeat_interleave(L)
        offs = torch.arange(ng + 1, dtype=torch.int64, device=dev) * L
        return ListColumn(offs, Column(T.F64, out, None), None,
                          T.ArrayType(T.F64))

    if name == "histogram_numeric":
        # Ben-Haim/Tom-Tov style: merge the closest centroid pair until
        # nb bins remain (ref: sail-function aggregate/histogram_numeric)
        from .column import ListColumn, StructColumn

        nb = int(args[1].to_pylist()[0]) if len(args) > 1 and len(args[1]) else 10
        vals = c.data[mask].to(torch.float64)
        if isinstance(c.dtype, T.DecimalType):
            vals = vals / (10.0 ** c.dtype.scale)
        g = gid[mask]
        import collections

        groups = collections.defaultdict(lambda: collections.Counter())
        for gg, vv in zip(g.tolist(), vals.tolist()):
            groups[gg][vv] += 1
        rows = [[] for _ in range(ng)]
        for k, cnt in groups.items():
            bins = sorted((x, float(y)) for x, y in cnt.items())
            while len(bins) > nb:
                gaps = [(bins[i + 1][0] - bins[i][0], i)
                        for i in range(len(bins) - 1)]
                _, i = min(gaps)
                (x1, y1), (x2, y2) = bins[i], bins[i + 1]
                bins[i:i + 2] = [((x1 * y1 + x2 * y2) / (y1 + y2), y1 + y2)]
            rows[k] = bins
        flat_x = [x for r in rows for x, _ in r]
        flat_y = [y for r in rows for _, y in r]
        offs = [0]
        for r in rows:
            offs.append(offs[-1] + len(r))
        elem = T.StructType((T.StructField("x", T.F64),
                             T.StructField("y", T.F64)))
        child = StructColumn(
            [("x", Column.from_values(flat_x, T.F64, device=dev)),
             ("y", Column.from_values(flat_y, T.F64, device=dev))],
            dtype=elem)
        return ListColumn(torch.tensor(offs, dtype=torch.int64, device=dev),
                          child, None, T.ArrayType(elem))

    if name in ("median", "percentile", "percentile_approx"):
        # exact median/percentile via host (small group counts expected)
        vals = c.data[mask].to(torch.float64)
        if isinstance(c.dtype, T.DecimalType):
            vals = vals / (10.0 ** c.dtype.scale)
        out = torch.zeros(ng, dtype=torch.float64, device=dev)
        g = gidm
        # simple per-group via host loop fallback (reference correctness path)
        import numpy as np

        gnp = g.cpu().numpy()
        vnp = vals.cpu().numpy()
        q = 0.5
        if name != "median" and len(args) > 1 and len(args[1]):
            q = float(args[1].to_pylist()[0])
        if name != "median" and len(args) > 2 and len(args[2]) \
                and bool(args[2].to_pylist()[0]):
            q = 1.0 - q  # WITHIN GROUP (ORDER BY x DESC)
        import collections

        groups = collections.defaultdict(list)
        for gg, vv in zip(gnp, vnp):
            groups[int(gg)].append(vv)
        res = np.zeros(ng)
        for k, lst in groups.items():
            res[k] = float(np.percentile(lst, q * 100))
        return Column(T.F64, torch.from_numpy(res).to(dev), None)

    if name == "approx_count_distinct":
        # exact distinct count (an exact answer satisfies the approx
        # contract; the reference's HLL sketch is a space tradeoff this
        # engine doesn't need at whole-partition scale)
        return agg_eval("count", args, gid, ng, True, filter_mask, T.I64)

    if name in ("corr", "covar_samp", "covar_pop", "regr_count", "regr_avgx",
                "regr_avgy", "regr_slope", "regr_intercept", "regr_r2",
                "regr_sxx", "regr_syy", "regr_sxy"):
        # Spark argument order: f(y, x) — args[0] is the DEPENDENT variable
        y = args[0]
        x = args[1]
        m = mask & x.valid_mask()
        gm = gid[m]
        xv = x.data[m].to(torch.float64)
        yv = y.data[m].to(torch.float64)
        if isinstance(x.dtype, T.DecimalType):
            xv = xv / (10.0 ** x.dtype.scale)
        if isinstance(y.dtype, T.DecimalType):
            yv = yv / (10.0 ** y.dtype.scale)

        def seg(v):
            o = torch.zeros(ng, dtype=torch.float64, device=dev)
            o.index_add_(0, gm, v)
            return o

        cnt = seg(torch.ones(gm.shape[0], dtype=torch.float64, device=dev))
        sx, sy = seg(xv), seg(yv)
        sxx, syy, sxy = seg(xv * xv), seg(yv * yv), seg(xv * yv)
        cn = cnt.clamp_min(1)
        mx, my = sx / cn, sy / cn
        cxx = sxx - cnt * mx * mx
        cyy = syy - cnt * my * my
        cxy = sxy - cnt * mx * my
        if name == "regr_count":
            return Column(T.I64, cnt.to(torch.int64), None)
        if name == "regr_avgx":
            data, valid = mx, cnt > 0
        elif name == "regr_avgy":
            data, valid = my, cnt > 0
        elif name == "regr_sxx":
            data, valid = cxx, cnt > 0
        elif name == "regr_syy":
            data, valid = cyy, cnt > 0
        elif name == "regr_sxy":
            data, valid = cxy, cnt > 0
        elif name == "regr_slope":
            data, valid = cxy / cxx.clamp_min(1e-300), (cnt > 0) & (cxx > 0)
        elif name == "regr_intercept":
            data = my - (cxy / cxx.clamp_min(1e-300)) * mx
            valid = (cnt > 0) & (cxx > 0)
        elif name == "regr_r2":
            data = (cxy * cxy) / (cxx * cyy).clamp_min(1e-300)
            valid = (cnt > 0) & (cxx > 0) & (cyy > 0)
        elif name == "corr":
            data = cxy / torch.sqrt((cxx * cyy).clamp_min(1e-300))
            valid = (cnt > 1) & (cxx > 0) & (cyy > 0)
        else:  # covar_samp / covar_pop
            denom = cnt - (1.0 if name == "covar_samp" else 0.0)
            data = cxy / denom.clamp_min(1e-300)
            valid = denom > 0
        return Column(T.F64, data,
                      None if bool(valid.all()) else valid.to(torch.uint8))

    if name in ("skewness", "kurtosis"):
        vals = c.data[mask].to(torch.float64)
        if isinstance(c.dtype, T.DecimalType):
            vals = vals / (10.0 ** c.dtype.scale)

        def seg(v):
            o = torch.zeros(ng, dtype=torch.float64, device=dev)
            o.index_add_(0, gidm, v)
            return o

        cnt = seg(torch.ones(n_used, dtype=torch.float64, device=dev))
        s1 = seg(vals)
        mu = s1 / cnt.clamp_min(1)
        d = vals - mu[gidm]
        m2 = seg(d * d) / cnt.clamp_min(1)
        m3 = seg(d * d * d) / cnt.clamp_min(1)
        m4 = seg(d * d * d * d) / cnt.clamp_min(1)
        if name == "skewness":
            data = m3 / m2.clamp_min(1e-300) ** 1.5
            valid = (cnt > 0) & (m2 > 0)
        else:  # Spark kurtosis: excess kurtosis
            data = m4 / (m2 * m2).clamp_min(1e-300) - 3.0
            valid = (cnt > 0) & (m2 > 0)
        return Column(T.F64, data,
                      None if bool(valid.all()) else valid.to(torch.uint8))

    if name in ("min_by", "max_by", "mode"):
        # sort by (gid, order-key) and take the first per group
        if name == "mode":
            vkey = normalize_key(c)[mask]
        else:
            ordc = args[1]
            m2 = mask & ordc.valid_mask()
            if not bool(m2.equal(mask)):
                mask = m2
            vkey = normalize_key(ordc)[mask]
        gm = gid[mask]
        rows = torch.nonzero(mask, as_tuple=False).flatten()
        if name == "mode":
            # count per (gid, value): sort then run lengths, keep max
            o1 = torch.argsort(vkey, stable=True)
            o2 = torch.argsort(gm.index_select(0, o1), stable=True)
            order = o1.index_select(0, o2)
            gs = gm.index_select(0, order)
            vs = vkey.index_select(0, order)
            nn = gs.shape[0]
            newrun = torch.ones(nn, dtype=torch.bool, device=dev)
            if nn > 1:
                newrun[1:] = (gs[1:] != gs[:-1]) | (vs[1:] != vs[:-1])
            run_id = torch.cumsum(newrun.to(torch.int64), 0) - 1
            nrun = int(run_id[-1].item()) + 1 if nn else 0
            rcnt = torch.zeros(nrun, dtype=torch.int64, device=dev)
            rcnt.index_add_(0, run_id, torch.ones(nn, dtype=torch.int64, device=dev))
            rgid = gs[newrun]
            rrow = rows.index_select(0, order)[newrun]
            best = torch.zeros(ng, dtype=torch.int64, device=dev)
            best.scatter_reduce_(0, rgid, rcnt, reduce="amax", include_self=True)
            pick = rcnt == best[rgid]
            # first winning run per group (large init: amin with include_self)
            sel_row = torch.full((ng,), 1 << 62, dtype=torch.int64, device=dev)
            cand = torch.nonzero(pick, as_tuple=False).flatten()
            sel_row.scatter_reduce_(0, rgid[cand], rrow[cand], reduce="amin",
                                    include_self=True)
            got = c.gather(sel_row.clamp(0, max(len(c) - 1, 0)))
            return got
        desc = name == "max_by"
        o1 = torch.argsort(vkey, stable=True, descending=desc)
        o2 = torch.argsort(gm.index_select(0, o1), stable=True)
        order = o1.index_select(0, o2)
        gs = gm.index_select(0, order)
        nn = gs.shape[0]
        first = torch.ones(nn, dtype=torch.bool, device=dev)
        if nn > 1:
            first[1:] = gs[1:] != gs[:-1]
        sel = rows.index_select(0, order)[first]
        # sel is ordered by group id; groups with no rows keep row 0 (masked
        # to null below)
        out_rows = torch.zeros(ng, dtype=torch.int64, device=dev)
        out_rows[gs[first]] = sel
        present = torch.zeros(ng, dtype=torch.bool, device=dev)
        present[gs[first]] = True
        got = c.gather(out_rows)
        vm = got.valid_mask() & present
        v = None if bool(vm.all()) else vm.to(torch.uint8)
        if isinstance(got, StringColumn):
            got.validity = v
            return got
        return Column(got.dtype, got.data, v)

    if name in ("bit_and", "bit_or", "bit_xor"):
        vals = c.data[mask].to(torch.int64)
        gm = gid[mask]
        if name == "bit_xor":
            # xor is addition mod 2 per bit: sum each bit's parity
            out = torch.zeros(ng, dtype=torch.int64, device=dev)
            for b in range(64):
                bit = (vals >> b) & 1
                acc = torch.zeros(ng, dtype=torch.int64, device=dev)
                acc.index_add_(0, gm, bit)
                out |= (acc & 1) << b
            return Column(T.I64, out, None)
        # and/or per bit via any/all (amax/amin of the bit)
        out = torch.zeros(ng, dtype=torch.int64, device=dev)
        red = "amin" if name == "bit_and" else "amax"
        for b in range(64):
            bit = (vals >> b) & 1
            acc = torch.full((ng,), 1 if name == "bit_and" else 0,
                             dtype=torch.int64, device=dev)
            acc.scatter_reduce_(0, gm, bit, reduce=red, include_self=True)
            out |= (acc & 1) << b
        return Column(T.I64, out, None)

    if name in ("string_agg", "listagg"):
        lst = agg_eval("collect_list", [c], gid, ng, False, filter_mask, None)
        sep = ","
        if len(args) > 1:
            sv = args[1]
            sep = sv.to_pylist()[0] if len(sv) else ","
        joined = [None if v is None or not v else sep.join(str(x) for x in v)
                  for v in lst.to_pylist()]
        return StringColumn.from_pylist(joined, device=dev)

    raise NotImplementedError(f"aggregate {name}")


def _avg_result(sums: torch.Tensor, cnt: torch.Tensor, in_type: T.DataType, out_type) -> Column:
    dev = sums.device
    valid = cnt > 0
    safe = cnt.clamp_min(1)
    if isinstance(in_type, T.DecimalType):
        ot = out_type if isinstance(out_type, T.DecimalType) else T.DecimalType(38, min(in_type.scale + 4, 10))
        # sums at in.scale; result at ot.scale
        num = sums.to(torch.float64) * (10.0 ** (ot.scale - in_type.scale))
        data = torch.round(num / safe.to(torch.float64)).to(torch.int64)
        return Column(ot, data, None if bool(valid.all()) else valid.to(torch.uint8))
    data = sums.to(torch.float64) / safe.to(torch.float64)
    return Column(T.F64, data, None if bool(valid.all()) else valid.to(torch.uint8))


def global_ids(n: int, device) -> Tuple[torch.Tensor, int]:
    """gid tensor for a global (no GROUP BY) aggregate: all rows in group 0."""
    return torch.zeros(n, dtype=torch.int64, device=device), 1


# ---------------------------------------------------------------------------
# fused GPU aggregation (ops/csrc/hash_agg.hip)
# ---------------------------------------------------------------------------

def agg_global_enabled() -> bool:
    """SAIL_EXEC_AGG_GLOBAL (config sail.exec.agg_global), default on: a
    GROUP BY above 4096 groups and direct-address aggregation go through
    grouped_acc_global. `off`, `0` or `false` selects the torch calls. Read on
    every aggregate, so one process can alternate the two."""
    v = os.environ.get("SAIL_EXEC_AGG_GLOBAL")
    return v is None or v.lower() not in ("off", "false", "0")


def _global_ext():
    """The extension when grouped_acc_global may be used, else None."""
    from ..ops import kernels as K

    if not agg_global_enabled() or not K.available():
        return None
    ext = K.require()
    return ext if hasattr(ext, "grouped_acc_global") else None


def _acc_global(ext, gid, mask, vals, ops, ng):
    """One grouped_acc_global launch. The kernel takes bool masks and every
    column dtype as stored; it only insists on contiguous memory."""
    vals = [v if v is None else v.contiguous() for v in vals]
    mask = mask if mask is None else mask.contiguous()
    return ext.grouped_acc_global(gid, mask, vals, ops, ng)


# ---------------------------------------------------------------------------
# COUNT / SUM / AVG (DISTINCT x) (ops/csrc/distinct_agg.hip)
# ---------------------------------------------------------------------------

def distinct_hash_enabled() -> bool:
    """SAIL_EXEC_DISTINCT_HASH (config sail.exec.distinct_hash), default on:
    count/sum/avg DISTINCT on the device go through distinct_acc, one pass
    over a hash set of (group, value) pairs. `off`, `0` or `false` selects the
    two sorts. Read at each use, so one process can alternate the two."""
    v = os.environ.get("SAIL_EXEC_DISTINCT_HASH")
    return v is None or v.lower() not in ("off", "false", "0")


# which way each distinct count/sum/avg went: `hash` (distinct_acc) or `sort`
# (two argsorts and index_add_: a host column, the switch off, a float sum, a
# table above half of the free device memory)
DISTINCT_PATHS = {"hash": 0, "sort": 0}
LAST_DISTINCT_PATH: Optional[str] = None


def _took_distinct(path: str) -> None:
    global LAST_DISTINCT_PATH
    DISTINCT_PATHS[path] += 1
    LAST_DISTINCT_PATH = path


_INT_STORAGE = (torch.int8, torch.int16, torch.int32, torch.int64)


def _distinct_ext(name: str, c: Column, gid: torch.Tensor, ng: int):
    """The extension when distinct_acc may serve this aggregate, else None."""
    n = gid.shape[0]
    if not gid.is_cuda or not distinct_hash_enabled() or n >= (1 << 32) - 1 \
            or not 1 <= ng < (1 << 31):
        return None
    if name != "count" and (isinstance(c, StringColumn) or c.data.dtype not in _INT_STORAGE):
        return None  # sums of ints, decimals and dates only
    from ..ops import kernels as K

    if not K.available():
        return None
    ext = K.require()
    if not hasattr(ext, "distinct_acc"):
        return None
    # the table: 2n slots rounded up to a power of two, 8 B each for one
    # group and 4 B otherwise; above half of the free memory the sorts stay.
    # The driver is asked only for tables above 256 MiB: the query costs more
    # than a small aggregate, and the sorts need several times the table
    slots = max(64, 1 << (2 * n - 1).bit_length()) if n else 64
    table = slots * (8 if ng == 1 else 4)
    if table > (1 << 28) and table > torch.cuda.mem_get_info(gid.device)[0] // 2:
        return None
    return ext


def _distinct_hash(ext, c: Column, gid: torch.Tensor, ng: int, mask: torch.Tensor,
                   want_sum: bool) -> torch.Tensor:
    """One distinct_acc launch -> int64 [2, ng]: distinct count, distinct sum."""
    _took_distinct("hash")
    return ext.distinct_acc(None if ng == 1 else gid.contiguous(),
                            normalize_key(c).contiguous(), mask.contiguous(), ng, want_sum)


# ---------------------------------------------------------------------------
# median / percentile / percentile_disc (ops/csrc/grouped_select.hip)
# ---------------------------------------------------------------------------

def percentile_select_enabled() -> bool:
    """SAIL_EXEC_PERCENTILE_SELECT (config sail.exec.percentile_select),
    default on: median, percentile and percentile_disc over a device column
    stay on the device (grouped_select, or two sorts above its histogram
    budget). `off`, `0` or `false` selects the host loop. Read at each use, so
    one process can alternate them."""
    v = os.environ.get("SAIL_EXEC_PERCENTILE_SELECT")
    return v is None or v.lower() not in ("off", "false", "0")


# which way each median/percentile went: `select` (grouped_select), `sort`
# (device sorts: more groups than the histogram budget holds) or `host` (a
# host column, the switch off, non-numeric input, no extension)
PERCENTILE_PATHS = {"select": 0, "sort": 0, "host": 0}
LAST_PERCENTILE_PATH: Optional[str] = None

#: bytes of grouped_select's [ng][256] uint32 bins above which `sort` serves
#: (the binding's own limit; tools/percentile_bench.py is where it comes from)
PERCENTILE_HIST_BUDGET = 1 << 28


def _took_percentile(path: str) -> None:
    global LAST_PERCENTILE_PATH
    PERCENTILE_PATHS[path] += 1
    LAST_PERCENTILE_PATH = path


def _percentile_device(name: str, args: List[Column], c: Column, gid: torch.Tensor, ng: int,
                       mask: torch.Tensor) -> Optional[Column]:
    """median / percentile / percentile_disc without leaving the device, or
    None where the host code has to serve."""
    n = gid.shape[0]
    if not gid.is_cuda or not percentile_select_enabled() or type(c) is not Column \
            or c.data.dtype not in _INT_STORAGE + (torch.float32, torch.float64) \
            or n == 0 or n >= (1 << 32) - 1 or ng < 1:
        return None
    from ..ops import kernels as K

    ext = K.require() if K.available() else None
    if not hasattr(ext, "grouped_select"):
        return None
    disc = name == "percentile_disc"
    q = 0.5
    if name != "median" and len(args) > 1 and len(args[1]):
        q = float(args[1].to_pylist()[0])
    desc = name != "median" and len(args) > 2 and len(args[2]) and bool(args[2].to_pylist()[0])
    if not disc and desc:
        q = 1.0 - q  # WITHIN GROUP (ORDER BY x DESC)
    if not 0.0 <= q <= 1.0:
        return None  # the host code words the error
    mode = 0 if not disc else (2 if desc else 1)
    qq = (q * 100) / 100  # numpy's own rounding of the percentage
    vals = c.data.to(torch.float64)
    if isinstance(c.dtype, T.DecimalType) and not disc:
        vals = vals / (10.0 ** c.dtype.scale)
    if ng * 1024 <= PERCENTILE_HIST_BUDGET:
        _took_percentile("select")
        lo_hi, meta = ext.grouped_select(vals.contiguous(), None if ng == 1 else gid.contiguous(),
                                         mask.contiguous(), ng, q, mode, qq)
        lo, hi, cnt, row, nan = lo_hi[0], lo_hi[1], meta[0], meta[1].clamp_min(0), meta[2] != 0
    else:
        _took_percentile("sort")
        lo, hi, cnt, row, nan = _percentile_sort(vals, gid, ng, mask, q, qq, mode)

    if disc:
        out = c.gather(row)
        has = cnt > 0
        if not bool(has.all()):
            out = Column(out.dtype, out.data, (out.valid_mask() & has).to(torch.uint8))
        return out
    # numpy's linear rule, one rounding per step as numpy has it
    vi = qq * (cnt - 1).clamp_min(0).to(torch.float64)
    t = vi - torch.floor(vi)
    d = hi - lo
    r = torch.where(t >= 0.5, hi - d * (1 - t), lo + d * t)
    r = torch.where(nan, torch.full_like(r, float("nan")), r)
    return Column(T.F64, torch.where(cnt == 0, torch.zeros_like(r), r), None)


def _percentile_sort(vals, gid, ng, mask, q, qq, mode):
    """What grouped_select returns, from two device sorts: rows ordered by
    (group, value, row), group starts from a bincount, two gathers."""
    rows = torch.nonzero(mask, as_tuple=False).flatten()
    v, g = vals[rows], gid[rows]
    o = torch.argsort(v, stable=True)            # NaNs last, as numpy sorts them
    o = o[torch.argsort(g[o], stable=True)]
    v, rows = v[o], rows[o]
    cnt = torch.bincount(g, minlength=ng)
    start = torch.cumsum(cnt, 0) - cnt
    last = (cnt - 1).clamp_min(0)
    if mode == 0:
        k = torch.floor(qq * last.to(torch.float64)).to(torch.int64)
    else:
        k = (torch.ceil(q * cnt.to(torch.float64)) - 1).to(torch.int64).clamp_min(0)
    k = torch.minimum(k, last)
    if mode == 2:
        k = last - k
    if v.numel() == 0:
        z = torch.zeros(ng, dtype=torch.float64, device=vals.device)
        return z, z, cnt, cnt, cnt != 0
    top = v.numel() - 1
    at = lambda i: (start + i).clamp_max(top)    # an empty group reads any row
    return (v[at(k)], v[at(torch.minimum(k + 1, last))], cnt, rows[at(k)],
            torch.isnan(v[at(last)]) & (cnt > 0))


def _distinct_finish(name: str, acc: torch.Tensor, c: Column, out_type) -> Column:
    if name == "count":
        return Column(T.I64, acc[0], None)
    if name == "avg":
        return _avg_result(acc[1], acc[0], c.dtype, out_type)
    return Column(out_type or T.I64, acc[1], None)


def fused_agg_batch(aggs, args_list, fmasks, gid: torch.Tensor, ng: int):
    """Evaluate a whole aggregate list in one (or few) fused kernel passes:
    grouped_acc up to 4096 groups, grouped_acc_global above. A DISTINCT
    count/sum/avg in the list is one distinct_acc launch of its own.

    aggs: list of S.AggFunc; args_list[i]: evaluated arg Columns;
    fmasks[i]: optional bool mask (FILTER clause). Returns list[Column] or
    None when ineligible (falls back to per-agg torch path).
    """
    if not gid.is_cuda or ng == 0:
        return None
    from ..ops import kernels as K

    if not K.available():
        return None
    ext = K.require()
    use_global = ng > 4096
    if use_global and (ng >= 1 << 31 or _global_ext() is None):
        return None

    n = gid.shape[0]
    # plan columns: per agg -> list of (value_tensor|None, op) + finalizer
    launches = {}  # key: id of fmask tensor (None -> 0) -> list of col specs
    plans = []
    for a, args, fm in zip(aggs, args_list, fmasks):
        name = a.name
        if a.distinct and name in ("count", "sum", "avg") and args:
            if _distinct_ext(name, args[0], gid, ng) is None:
                return None
            plans.append(("distinct", None, None, (args[0], fm), a))
            continue
        if a.distinct or name not in ("sum", "try_sum", "count", "count_if",
                                      "avg", "try_avg", "min", "max"):
            return None
        c = args[0] if args else None
        if c is not None and isinstance(c, StringColumn) and not c.is_dict:
            return None
        if c is not None and c.dtype.is_float and name in ("min", "max"):
            return None  # float min/max: bit-cast doesn't order negatives
        mkey = id(fm) if fm is not None else 0
        cols = launches.setdefault(mkey, (fm, []))[1]

        def add(spec):
            cols.append(spec)
            return len(cols) - 1

        if name in ("count", "count_if"):
            if name == "count_if":
                vt = (c.data.to(torch.uint8) if c.data.dtype == torch.bool else c.data)
                if c.validity is not None:
                    vt = vt * c.validity
                idx = add((vt, 0))
            elif c is None or c.validity is None:
                idx = add((None, 2))
            else:
                idx = add((c.validity, 0))
            plans.append(("count", mkey, idx, None, a))
            continue
        if name in ("sum", "try_sum", "avg", "try_avg"):
            is_f = c.dtype.is_float
            data = c.data
            if c.validity is not None:
                data = data * c.validity.to(data.dtype)
            if is_f:
                vidx = add((data.to(torch.float64), 1))
            else:
                # overflow check: int64 accumulation only when safe
                amax = int(data.abs().max().item()) if n else 0
                if amax and amax > (1 << 62) // max(n, 1):
                    vidx = add((data.to(torch.float64), 1))
                    is_f = True
                else:
                    vidx = add((data, 0))
            cidx = None
            if name in ("avg", "try_avg") or c.validity is not None or fm is not None:
                cidx = add((c.validity, 0) if c.validity is not None else (None, 2))
            plans.append(("sumavg", mkey, vidx, (cidx, is_f, c.dtype), a))
            continue
        # min/max
        if isinstance(c, StringColumn):
            data = c.codes
        else:
            data = c.data
        if c.validity is not None:
            return None  # rare; keep torch path for nullable min/max
        op = 3 if name == "min" else 4
        vidx = add((data, op))
        plans.append(("minmax", mkey, vidx, (op, c), a))

    # grouped_acc_global reads int64 ids as they are
    gid_k = gid.contiguous() if use_global else gid.to(torch.int32)
    results = {}
    for mkey, (fm, cols) in launches.items():
        outs = []
        # <=4 columns per launch: the register-accumulated tiny variant
        # needs NC*8 int64 accumulators per thread; 10 columns tanks
        # occupancy (measured 180 GB/s vs ~1 TB/s at 4 columns)
        for i in range(0, len(cols), 4):
            chunk_cols = cols[i : i + 4]
            vals = [t for t, _ in chunk_cols]
            ops = [int(op) for _, op in chunk_cols]
            if use_global:
                out = _acc_global(ext, gid_k, fm, vals, ops, ng)
            else:
                mask_t = fm.to(torch.uint8) if fm is not None and fm.dtype == torch.bool else fm
                out = ext.grouped_acc(gid_k, mask_t, vals, ops, ng)
            outs.extend(out[j] for j in range(out.shape[0]))
        results[mkey] = outs

    # finalize per agg
    out_cols: List[Column] = []
    for kind, mkey, vidx, extra, a in plans:
        if kind == "distinct":
            c, fm = extra  # its own mask: validity & FILTER
            acc = _distinct_hash(ext, c, gid, ng, _masked(c, fm), a.name != "count")
            out_cols.append(_distinct_finish(a.name, acc, c, a.dtype))
            continue
        outs = results[mkey]
        if kind == "count":
            out_cols.append(Column(T.I64, outs[vidx]))
        elif kind == "sumavg":
            cidx, is_f, in_type = extra
            acc = outs[vidx]
            accv = acc.view(torch.float64) if is_f else acc
            cnt = outs[cidx] if cidx is not None else None
            if a.name in ("avg", "try_avg"):
                if is_f and not isinstance(in_type, T.DecimalType):
                    out_cols.append(_avg_result(accv, cnt, T.F64, a.dtype))
                else:
                    sums = accv
                    if is_f and isinstance(in_type, T.DecimalType):
                        sums = torch.round(accv).to(torch.int64)
                    out_cols.append(_avg_result(sums, cnt, in_type, a.dtype))
            else:
                rt = a.dtype or (T.I64 if not isinstance(in_type, T.DecimalType) and not in_type.is_float else in_type)
                if isinstance(in_type, T.DecimalType):
                    data = torch.round(accv).to(torch.int64) if is_f else accv
                    if isinstance(rt, T.DecimalType) and rt.scale != in_type.scale:
                        from .eval import _rescale_int

                        data = _rescale_int(data, in_type.scale, rt.scale)
                    col = Column(rt, data)
                elif in_type.is_float:
                    col = Column(T.F64, accv.view(torch.float64) if not is_f else accv)
                else:
                    col = Column(T.I64, accv)
                if cnt is not None:
                    zero = cnt == 0
                    if bool(zero.any()):
                        col.validity = (~zero).to(torch.uint8)
                out_cols.append(col)
        else:  # minmax
            op, c = extra
            acc = outs[vidx]
            sentinel = (1 << 63) - 1 if op == 3 else -(1 << 63)
            valid = acc != sentinel
            v = None if bool(valid.all()) else valid.to(torch.uint8)
            if isinstance(c, StringColumn):
                out_cols.append(StringColumn(c.offsets, c.bytes_, v, acc.to(torch.int32)))
            else:
                out_cols.append(Column(a.dtype or c.dtype,
                                       acc.to(c.data.dtype) if c.data.dtype != torch.int64 else acc, v))
    return out_cols


def _direct_accumulate_torch(packed, prepared, total):
    """try_direct_aggregate's tables, one index_add_ each. Returns the
    presence count and per aggregate (table, row count or None)."""
    dev = packed.device

    def count(mask):
        idx = packed if mask is None else packed[mask]
        acc = torch.zeros(total, dtype=torch.int64, device=dev)
        acc.index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.int64, device=dev))
        return acc

    cnt = count(None)
    accs = []
    for mask, data, _ in prepared:
        if data is None:
            accs.append((cnt if mask is None else count(mask), None))
            continue
        acc = torch.zeros(total, dtype=data.dtype, device=dev)
        if mask is None:
            acc.index_add_(0, packed, data)
            accs.append((acc, cnt))
        else:
            acc.index_add_(0, packed[mask], data[mask])
            accs.append((acc, count(mask)))
    return cnt, accs


def _direct_accumulate_fused(ext, packed, prepared, total):
    """The same tables from grouped_acc_global: one launch group per row
    mask, up to 4 columns per launch, each group's row count its column 0
    (for the unmasked group that is the presence count). The mask goes to the
    kernel, so nothing is compacted."""
    groups = {0: (None, [(None, 2)])}
    where = []
    for mask, data, is_f in prepared:
        key = 0 if mask is None else id(mask)
        cols = groups.setdefault(key, (mask, [(None, 2)]))[1]
        if data is not None:
            cols.append((data, 1 if is_f else 0))
        where.append(len(cols) - 1 if data is not None else 0)
    outs = {}
    for key, (mask, cols) in groups.items():
        rows = []
        for i in range(0, len(cols), 4):
            chunk = cols[i:i + 4]
            out = _acc_global(ext, packed, mask, [t for t, _ in chunk],
                              [op for _, op in chunk], total)
            rows.extend(out[j] for j in range(out.shape[0]))
        outs[key] = rows
    accs = []
    for (mask, data, is_f), idx in zip(prepared, where):
        rows = outs[0 if mask is None else id(mask)]
        if data is None:
            accs.append((rows[0], None))
        else:
            accs.append((rows[idx].view(torch.float64) if is_f else rows[idx], rows[0]))
    return outs[0][0], accs


DIRECT_MIN_ROWS = 1_000_000


def try_direct_aggregate(key_cols: List[Column], aggs, args_list, fmasks):
    """Direct-address aggregation for dense high-cardinality keys
    (150M l_orderkey groups in q18): accumulate straight into a span-sized
    table (grouped_acc_global launches of up to 4 columns, or index_add
    without the kernel) and compact once — skips the whole gid machinery
    (presence bitmap + cumsum + lut gather + representative scatter were 4
    extra random passes over 600M rows). Key VALUES are reconstructed
    arithmetically from the slot index, so no representative gather either.
    Group order equals the packed-value order — identical to the dense
    group_ids path. Returns (key_cols_out, agg_cols) or None."""
    if not key_cols:
        return None
    n = len(key_cols[0])
    if n < DIRECT_MIN_ROWS:
        return None
    for c in key_cols:
        if c.validity is not None:
            return None  # null keys: use the generic path
    for a, args in zip(aggs, args_list):
        if a.distinct or a.name not in ("sum", "try_sum", "count", "count_if",
                                        "avg", "try_avg"):
            return None
        if args and isinstance(args[0], StringColumn):
            return None
    norm = [normalize_key(c) for c in key_cols]
    mins, spans = [], []
    total = 1
    for k in norm:
        lo = int(k.min().item())
        hi = int(k.max().item())
        mins.append(lo)
        spans.append(hi - lo + 1)
        total *= spans[-1]
        if total > max(4 * n, 1 << 22) or total > (1 << 31):
            return None
    if total <= 4096:
        return None  # tiny/LDS grouped_acc kernels handle this better
    packed = norm[0] - mins[0]
    for i in range(1, len(norm)):
        packed = packed * spans[i] + (norm[i] - mins[i])

    # per aggregate: its row mask and, for sum / avg, the values to add
    prepared = []
    for a, args, fm in zip(aggs, args_list, fmasks):
        c = args[0] if args else None
        mask = None
        if c is not None and c.validity is not None:
            mask = c.valid_mask()
        if fm is not None:
            mask = fm if mask is None else (mask & fm)
        if a.name in ("count", "count_if"):
            if a.name == "count_if":
                m2 = c.data.to(torch.bool)
                mask = m2 if mask is None else (mask & m2)
            prepared.append((mask, None, False))
            continue
        data = c.data
        if data.dtype == torch.bool:
            data = data.to(torch.int64)
        is_f = data.dtype.is_floating_point
        if not is_f:
            amax = int(data.abs().max().item()) if n else 0
            if amax and amax > (1 << 62) // max(n, 1):
                data = data.to(torch.float64)
                is_f = True
            elif data.dtype != torch.int64:
                data = data.to(torch.int64)
        else:
            data = data.to(torch.float64)
        prepared.append((mask, data, is_f))

    # the kernel takes G < 2^31; a span of exactly 2^31 stays on index_add_
    ext = _global_ext() if packed.is_cuda and total < (1 << 31) else None
    if ext is not None:
        cnt, accs = _direct_accumulate_fused(ext, packed, prepared, total)
    else:
        cnt, accs = _direct_accumulate_torch(packed, prepared, total)
    present = cnt > 0
    out_idx = torch.nonzero(present, as_tuple=False).flatten()

    # reconstruct key columns from the slot index
    out_keys: List[Column] = []
    rem = out_idx
    for i, c in enumerate(key_cols):
        stride = 1
        for s in spans[i + 1:]:
            stride *= s
        code = rem // stride + mins[i]
        rem = rem % stride if i < len(key_cols) - 1 else rem
        if isinstance(c, StringColumn):
            out_keys.append(StringColumn(c.offsets, c.bytes_, None,
                                         code.to(torch.int32), dtype=c.dtype))
        else:
            out_keys.append(Column(c.dtype, code.to(c.data.dtype), None))

    agg_cols: List[Column] = []
    for a, args, (_, data, is_f), (acc, gcnt) in zip(aggs, args_list, prepared, accs):
        name = a.name
        c = args[0] if args else None
        if data is None:
            agg_cols.append(Column(T.I64, acc.index_select(0, out_idx)))
            continue
        sums = acc.index_select(0, out_idx)
        if name in ("avg", "try_avg"):
            gc = gcnt.index_select(0, out_idx)
            if is_f and isinstance(c.dtype, T.DecimalType):
                sums = torch.round(sums).to(torch.int64)
            agg_cols.append(_avg_result(sums, gc, c.dtype if not is_f or
                                        isinstance(c.dtype, T.DecimalType) else T.F64,
                                        a.dtype))
        else:
            rt = a.dtype or (c.dtype if isinstance(c.dtype, T.DecimalType) or c.dtype.is_float else T.I64)
            if is_f and isinstance(c.dtype, T.DecimalType):
                sums = torch.round(sums).to(torch.int64)
            if isinstance(c.dtype, T.DecimalType) and isinstance(rt, T.DecimalType) \
                    and rt.scale != c.dtype.scale:
                from .eval import _rescale_int

                sums = _rescale_int(sums, c.dtype.scale, rt.scale)
            if rt.storage is not None and sums.dtype != rt.storage \
                    and not rt.is_float:
                sums = sums.to(rt.storage)
            agg_cols.append(Column(rt, sums, None))
    return out_keys, agg_cols
