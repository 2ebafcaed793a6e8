"""Arrow interop: Chunk <-> pyarrow (host boundary for clients/files)."""
from __future__ import annotations

import pyarrow as pa
import torch

from ..engine import types as T
from ..engine.chunk import Chunk
from ..engine.column import Column, StringColumn


def _arrow_type(t: T.DataType) -> pa.DataType:
    if isinstance(t, T.DecimalType):
        return pa.decimal128(max(t.precision, t.scale + 1), t.scale)
    if isinstance(t, T.ArrayType):
        return pa.large_list(_arrow_type(t.element))
    m = {T.BooleanType: pa.bool_(), T.Int8Type: pa.int8(), T.Int16Type: pa.int16(),
         T.Int32Type: pa.int32(), T.Int64Type: pa.int64(), T.Float32Type: pa.float32(),
         T.Float64Type: pa.float64(), T.DateType: pa.date32(),
         T.TimeType: pa.time64("us"),
         T.TimestampType: pa.timestamp("us"), T.StringType: pa.string(),
         T.BinaryType: pa.binary(), T.NullType: pa.null()}
    return m[type(t)]


def column_to_arrow(c: Column, t: T.DataType) -> pa.Array:
    import numpy as np

    from ..engine.column import ListColumn

    if isinstance(c, ListColumn):
        child = column_to_arrow(c.child, c.child.dtype)
        if isinstance(child, pa.DictionaryArray):
            child = child.cast(pa.large_string())
        offs = pa.array(c.offsets.cpu().numpy(), type=pa.int64())
        out = pa.LargeListArray.from_arrays(offs, child)
        if c.validity is not None:
            mask = pa.array(c.valid_mask().cpu().numpy())
            out = pa.LargeListArray.from_arrays(
                offs, child, mask=pa.compute.invert(mask))
        return out
    if isinstance(c, StringColumn):
        if c.is_dict:
            # keep dictionary encoding end-to-end (parquet dictionary pages)
            codes = c.codes.cpu().numpy()
            vals = _raw_string_array(c.offsets.cpu(), c.bytes_.cpu())
            mask = None
            if c.validity is not None:
                mask = ~c.validity.cpu().numpy().astype(bool)
            ind = pa.array(codes, type=pa.int32(), mask=mask)
            return pa.DictionaryArray.from_arrays(ind, vals)
        arr = _raw_string_array(c.offsets.cpu(), c.bytes_.cpu(),
                                validity=c.validity.cpu() if c.validity is not None else None)
        return arr
    data = c.data.cpu().numpy()
    mask = None
    if c.validity is not None:
        mask = ~c.validity.cpu().numpy().astype(bool)
    if isinstance(t, T.DecimalType):
        # vectorized int64 -> decimal128 (16-byte little-endian two's complement)
        lo = data.astype(np.int64)
        buf = np.zeros((len(lo), 2), dtype=np.int64)
        buf[:, 0] = lo
        buf[:, 1] = np.where(lo < 0, -1, 0)  # sign extension
        validity_buf = None
        if mask is not None:
            validity_buf = pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes())
        # zero-copy wrap (pa.py_buffer holds a reference to the ndarray)
        return pa.Array.from_buffers(_arrow_type(t), len(lo),
                                     [validity_buf, pa.py_buffer(buf)])
    return pa.array(data, type=_arrow_type(t), mask=mask)


def _raw_string_array(offsets, bytes_, validity=None) -> pa.Array:
    import numpy as np

    n = offsets.numel() - 1
    validity_buf = None
    if validity is not None:
        validity_buf = pa.py_buffer(
            np.packbits(validity.numpy().astype(bool), bitorder="little").tobytes())
    return pa.Array.from_buffers(
        pa.large_string(), n,
        [validity_buf, pa.py_buffer(offsets.contiguous().numpy()),
         pa.py_buffer(bytes_.contiguous().numpy())])


def chunk_to_arrow(chunk: Chunk, schema) -> pa.Table:
    arrays = []
    names = []
    for (n, t), c in zip(schema, chunk.columns):
        arrays.append(column_to_arrow(c, t))
        names.append(n)
    return pa.table(arrays, names=names)


def arrow_to_table(tbl: pa.Table, device="cpu", dict_encode=True):
    """pyarrow Table -> engine Table (host decode path)."""
    from ..engine.column import Table

    cols = {}
    for name, col in zip(tbl.column_names, tbl.columns):
        cols[name] = arrow_column(col, device, dict_encode)
    return Table(cols)


def arrow_column(col: pa.ChunkedArray, device="cpu", dict_encode=True) -> Column:
    import numpy as np

    at = col.type
    combined = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    if pa.types.is_dictionary(at):
        arr = combined.combine_chunks() if isinstance(combined, pa.ChunkedArray) else combined
        if pa.types.is_string(at.value_type) or pa.types.is_large_string(at.value_type):
            vals = arr.dictionary
            # engine invariant: dictionaries sorted — remap if needed
            import numpy as np

            pyvals = vals.to_pylist()
            order = sorted(range(len(pyvals)), key=lambda i: pyvals[i] if pyvals[i] is not None else "")
            sorted_vals = [pyvals[i] for i in order]
            remap = np.empty(len(pyvals), dtype=np.int32)
            for new, old in enumerate(order):
                remap[old] = new
            codes_np = arr.indices.to_numpy(zero_copy_only=False).astype(np.int64)
            nullmask = (codes_np < 0) | (codes_np >= len(pyvals))
            codes_np = np.where(nullmask, 0, codes_np)
            mapped = remap[codes_np].astype(np.int32)
            mapped = np.where(nullmask, np.int32(-1), mapped)
            codes = torch.from_numpy(mapped).to(device)
            from ..engine.column import _pack_strings

            offs, byts = _pack_strings([v or "" for v in sorted_vals], device)
            validity = _validity(arr, device)
            return StringColumn(offs, byts, validity, codes)
        combined = combined.cast(at.value_type)
        at = at.value_type
    if pa.types.is_string(at) or pa.types.is_large_string(at):
        return _string_from_arrow(combined, device)
    if pa.types.is_decimal(at):
        scale = at.scale
        arr = combined.combine_chunks() if isinstance(combined, pa.ChunkedArray) else combined
        # torch.frombuffer: numpy copies from pyarrow buffers run ~100x
        # slower on this platform (measured 53 MB/s vs 8 GB/s)
        raw = torch.frombuffer(arr.buffers()[1], dtype=torch.int64)
        lo = raw.view(-1, 2)[arr.offset : arr.offset + len(arr), 0].clone()
        data = lo.to(device)
        validity = _validity(arr, device)
        return Column(T.DecimalType(at.precision, scale), data, validity)
    npmap = {pa.bool_(): (torch.bool, T.BOOL), pa.int8(): (torch.int8, T.I8),
             pa.int16(): (torch.int16, T.I16), pa.int32(): (torch.int32, T.I32),
             pa.int64(): (torch.int64, T.I64), pa.float32(): (torch.float32, T.F32),
             pa.float64(): (torch.float64, T.F64), pa.date32(): (torch.int32, T.DATE)}
    if pa.types.is_timestamp(at):
        arr = combined.cast(pa.timestamp("us"))
        np_data = arr.to_numpy(zero_copy_only=False).astype("datetime64[us]").astype(np.int64)
        data = torch.from_numpy(np_data).to(device)
        validity = _validity(combined, device)
        return Column(T.TIMESTAMP, data, validity)
    for patype, (tt, et) in npmap.items():
        if at.equals(patype):
            arr = combined.combine_chunks() if isinstance(combined, pa.ChunkedArray) else combined
            if arr.offset != 0:
                arr = pa.concat_arrays([arr])
            if pa.types.is_date32(at):
                data = torch.frombuffer(arr.buffers()[1], dtype=torch.int32)[: len(arr)].clone().to(device)
            elif at.equals(pa.bool_()):
                # with nulls to_numpy would hand back objects; the null
                # slots are masked by the validity below
                np_data = arr.fill_null(False).to_numpy(zero_copy_only=False)
                data = torch.from_numpy(np.ascontiguousarray(np_data)).to(tt).to(device)
            else:
                data = torch.frombuffer(arr.buffers()[1], dtype=tt)[: len(arr)].clone().to(device)
            validity = _validity(arr, device)
            return Column(et, data, validity)
    raise ValueError(f"unsupported arrow type {at}")


def _string_from_arrow(arr: pa.Array, device) -> StringColumn:
    import numpy as np

    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if arr.offset != 0:
        # re-materialize so buffer offsets start at zero
        arr = pa.concat_arrays([arr])
    at = arr.type
    bufs = arr.buffers()
    if pa.types.is_large_string(at):
        offs = torch.frombuffer(bufs[1], dtype=torch.int64)[: len(arr) + 1].clone()
    else:
        offs = torch.frombuffer(bufs[1], dtype=torch.int32)[: len(arr) + 1].to(torch.int64)
    nb = int(offs[-1].item())
    byts = (torch.frombuffer(bufs[2], dtype=torch.uint8)[:nb].clone()
            if bufs[2] is not None and nb
            else torch.zeros(0, dtype=torch.uint8))
    validity = _validity(arr, device)
    return StringColumn(offs.to(device), byts.to(device), validity)


def _validity(arr: pa.Array, device):
    if arr.null_count == 0:
        return None
    m = pa.compute.is_valid(arr).to_numpy(zero_copy_only=False)
    return torch.from_numpy(m.astype("uint8")).to(device)
