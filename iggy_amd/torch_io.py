"""Copies between host numpy arrays and torch device tensors through pinned staging.

Plumbing for the Python callers of the codec that move their own buffers with torch
(the tests, smoke(), bench.py). The HIP runtime copies PAGEABLE host memory by page-
locking the caller's range on the fly (ROCclr, transfers above GPU_PINNED_MIN_XFER_SIZE).
On this pool that path faulted (hipErrorIllegalAddress inside a pageable copy) in rounds
3-5, once inside torch's own `.to("cuda")` with no codec call since the last stream
synchronisation. The codec never uses that path (host_mem.hpp put_host /
get_host stage pageable bytes through its own pinned chunks); these helpers keep the
callers' own copies off it too: a host memcpy into torch's pinned (hipHostMalloc) cache,
then a DMA from page-locked memory.
"""
from __future__ import annotations

import os

import numpy as np

# Diagnostics only: IGGY_TORCH_IO_PAGEABLE=1 restores torch's plain pageable copies (the
# path that faulted), to run the suite once under the round-5 conditions with the codec's
# host-memory history attached to any failure (tests/conftest.py).
_PAGEABLE = os.environ.get("IGGY_TORCH_IO_PAGEABLE") == "1"


def to_device(a, device="cuda"):
    """A device tensor holding a copy of the numpy array `a` (same dtype and shape)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if _PAGEABLE:
        return t.to(device)
    p = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    p.copy_(t)
    return p.to(device)


def unpack_record(cx, d_record, integrity: int = 0, cursor=None) -> dict:
    """Decode the device-resident record `d_record` (a uint8 CUDA tensor) and unpack it
    into struct-of-arrays torch tensors (iggy_codec_unpack_batch_device): decode and
    unpack are enqueued back to back on the current stream, then ONE synchronise.

    Returns a dict of tensors trimmed to the record's `count` messages: ids [count, 2],
    checksums, offsets, timestamps, origin_timestamps, payload_lengths,
    user_headers_lengths, payload_starts / user_headers_starts [count + 1], payloads,
    user_headers, plus `count`, `first_message` and, when every payload has one length L,
    `payloads_2d`, a [count, L] view of `payloads`. Raises CodecError carrying the wire
    error when the record does not decode (or an enqueue fails).

    cursor: an optional int64 CUDA tensor of 4 (an iggy_unpack_cursor) that this call
    advances; its totals are read first (one small copy) so that the arrays hold
    them, and the returned tensors are this record's part (the starts stay absolute)."""
    import ctypes

    import torch

    from . import abi
    from .codec import CodecError

    if d_record.dtype != torch.uint8 or not d_record.is_cuda or not d_record.is_contiguous():
        raise ValueError("d_record must be a contiguous uint8 CUDA tensor")
    n = d_record.numel()
    dev = d_record.device
    bm = bp = bu = 0
    if cursor is not None:
        bm, bp, bu = (int(x) for x in to_host(cursor)[:3])
    cap_m = n // 48 + 1
    cap_b = max(n - 256, 0)

    def arr(k, dtype):
        return torch.empty(max(k, 1), dtype=dtype, device=dev)

    i64 = torch.int64  # (torch has no uint64 arithmetic: the u64 arrays are int64 bit patterns)
    t = {
        "ids": arr(2 * (bm + cap_m), i64), "checksums": arr(bm + cap_m, i64), "offsets": arr(bm + cap_m, i64),
        "timestamps": arr(bm + cap_m, i64), "origin_timestamps": arr(bm + cap_m, i64),
        "payload_lengths": arr(bm + cap_m, torch.int32), "user_headers_lengths": arr(bm + cap_m, torch.int32),
        "payload_starts": arr(bm + cap_m + 1, i64), "user_headers_starts": arr(bm + cap_m + 1, i64),
        "payloads": arr(bp + cap_b, torch.uint8), "user_headers": arr(bu + cap_b, torch.uint8),
    }
    out = abi.UnpackedMessages(bm + cap_m, bp + cap_b, bu + cap_b, *(t[k].data_ptr() for k in (
        "ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
        "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")))
    d_pos = arr(cap_m, i64)
    d_dec = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(ctypes.sizeof(abi.UnpackResult), dtype=torch.uint8, device=dev)
    # torch's default stream is handle 0, which the C ABI reads as "the context's own
    # stream": then the work goes there, ordered after and before torch's stream by events
    cur = torch.cuda.current_stream(dev)
    work = cur if cur.cuda_stream else torch.cuda.ExternalStream(cx.stream(), device=dev)
    if work is not cur:
        work.wait_stream(cur)
    s = work.cuda_stream
    rc = cx.decode_device(d_record.data_ptr(), n, integrity, d_pos.data_ptr(), cap_m, d_dec.data_ptr(), s)
    if rc:
        raise CodecError(rc, None, "unpack_record: decode")
    rc = cx.unpack_device(d_record.data_ptr(), n, d_pos.data_ptr(), d_dec.data_ptr(), out,
                          cursor.data_ptr() if cursor is not None else None, d_res.data_ptr(), s)
    if rc:
        raise CodecError(rc, None, "unpack_record: unpack")
    if work is not cur:
        cur.wait_stream(work)
    res =abi.UnpackResult.from_buffer_copy(to_host(d_res).tobytes())  # the one synchronise
    if res.error.kind != abi.OK:
        raise CodecError(res.error.kind, res.error, "unpack_record")
    c, f = res.count, res.first_message
    r = {k: t[k][f:f + c] for k in ("checksums", "offsets", "timestamps", "origin_timestamps",
                                    "payload_lengths", "user_headers_lengths")}
    r["ids"] = t["ids"][2 * f:2 * (f + c)].view(c, 2)
    r["payload_starts"] = t["payload_starts"][f:f + c + 1]
    r["user_headers_starts"] = t["user_headers_starts"][f:f + c + 1]
    r["payloads"] = t["payloads"][bp:bp + res.payload_bytes]
    r["user_headers"] = t["user_headers"][bu:bu + res.user_headers_bytes]
    r["count"], r["first_message"] = c, f
    r["payload_base"], r["user_headers_base"] = bp, bu  # where the (absolute) starts begin
    if c and res.min_payload_length == res.max_payload_length:
        r["payloads_2d"] = r["payloads"].view(c, res.max_payload_length)
    return r


def header_columns(cx, d_record, keys, integrity: int = 0) -> dict:
    """Decode the device-resident record `d_record` (a uint8 CUDA tensor), validate every
    message's user headers and project the requested keys into per-message columns
    (iggy_codec_user_headers_device): decode and columns are enqueued back to back on the
    current stream, then ONE synchronise.

    keys: up to 16 (kind, key bytes) pairs, kind an abi.KIND_* code. Returns a dict of
    tensors trimmed to the record's `count` messages: `status` [count, 4] int32 (kind,
    reason, offset, detail of iggy_header_status), `pairs` [count] int32, and `columns`, one
    dict per key with `value_kinds` [count] uint8 (0 = absent), `value_lengths` [count]
    uint8, `value_pos` [count] int32 and `values16` [count, 16] uint8 (the value's bytes as
    stored, zero-padded); plus `count`, `with_headers`, `invalid_messages`, `first_invalid`
    (None if every message is valid) and `found` (one count per key).

    A fixed-size value is read by viewing its column, e.g. an Int64 / Uint64 / Float64 key:
        col["values16"].view(torch.int64)[:, 0]      # (.view(torch.float64) for Float64)
    and an Int32 key: col["values16"].view(torch.int32)[:, 0]; rows where value_kinds is 0
    (absent key, or invalid headers) hold zeros.

    The arrays form runs over what unpack_record wrote, e.g. several records chained with
    one cursor (an int64 CUDA tensor of 4) and one call over all of them:
        parts = [unpack_record(cx, r, cursor=cursor) for r in records]
        # with `uh`, `starts` the whole user_headers / user_headers_starts arrays
        cx.user_headers_arrays_device(uh.data_ptr(), starts.data_ptr(), cursor.data_ptr(),
                                      cap, q, d_result.data_ptr(), stream)
    (the cursor's first word is its `messages`, read on the device).
    Raises CodecError carrying the wire error when the record does not decode."""
    import ctypes

    import torch

    from . import abi
    from .codec import CodecError

    if d_record.dtype != torch.uint8 or not d_record.is_cuda or not d_record.is_contiguous():
        raise ValueError("d_record must be a contiguous uint8 CUDA tensor")
    keys = list(keys)
    if len(keys) > abi.HEADER_MAX_KEYS:
        raise ValueError("at most 16 keys")
    n = d_record.numel()
    dev = d_record.device
    cap = n // 48 + 1

    def arr(shape, dtype):
        return torch.empty(shape, dtype=dtype, device=dev)

    status, pairs = arr((cap, 4), torch.int32), arr((cap,), torch.int32)
    cols = [{"value_kinds": arr((cap,), torch.uint8), "value_lengths": arr((cap,), torch.uint8),
             "value_pos": arr((cap,), torch.int32), "values16": arr((cap, 16), torch.uint8)} for _ in keys]
    q = abi.HeaderColumns()
    q.cap_messages, q.nkeys = cap, len(keys)
    q.status, q.pairs = status.data_ptr(), pairs.data_ptr()
    for k, (kind, key) in enumerate(keys):
        q.keys[k] = abi.HeaderKey.make(kind, key)
        q.columns[k] = abi.HeaderColumn(*(cols[k][f].data_ptr() for f in ("value_kinds", "value_lengths",
                                                                           "value_pos", "values16")))
    d_pos = arr((cap,), torch.int64)
    d_dec = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(ctypes.sizeof(abi.HeaderColumnsResult), dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev)  # (stream handling as unpack_record)
    work = cur if cur.cuda_stream else torch.cuda.ExternalStream(cx.stream(), device=dev)
    if work is not cur:
        work.wait_stream(cur)
    s = work.cuda_stream
    rc = cx.decode_device(d_record.data_ptr(), n, integrity, d_pos.data_ptr(), cap, d_dec.data_ptr(), s)
    if rc:
        raise CodecError(rc, None, "header_columns: decode")
    rc = cx.user_headers_device(d_record.data_ptr(), n, d_pos.data_ptr(), d_dec.data_ptr(), q, d_res.data_ptr(), s)
    if rc:
        raise CodecError(rc, None, "header_columns: user headers")
    if work is not cur:
        cur.wait_stream(work)
    res = abi.HeaderColumnsResult.from_buffer_copy(to_host(d_res).tobytes())  # the one synchronise
    if res.error.kind != abi.OK:
        raise CodecError(res.error.kind, res.error, "header_columns")
    c = res.count
    return {
        "count": c, "with_headers": res.with_headers, "invalid_messages": res.invalid_messages,
        "first_invalid": None if res.first_invalid == 2**64 - 1 else res.first_invalid,
        "found": [res.found[k] for k in range(len(keys))],
        "status": status[:c], "pairs": pairs[:c],
        "columns": [{f: t[:c] for f, t in col.items()} for col in cols],
    }


_SEL_SOURCES = {"offset": 1, "timestamp": 2, "origin_timestamp": 3, "payload_length": 4, "user_headers_length": 5,
                "id": 6}
_SEL_OPS = {"==": 1, "!=": 2, "<": 3, "<=": 4, ">": 5, ">=": 6, "present": 7, "absent": 8}
_SEL_KIND_SIZE = {3: 1, 4: 1, 5: 2, 6: 4, 7: 8, 8: 16, 9: 1, 10: 2, 11: 4, 12: 8, 13: 16, 14: 4, 15: 8}


def select_clause(source, op=None, value=None, kind: int = 0):
    """One abi.SelectClause for select_messages.

    source: "offset", "timestamp", "origin_timestamp", "payload_length", "user_headers_length" or
    "id" with op one of "==", "!=", "<", "<=", ">", ">=" and an int value; or one column dict of
    header_columns()["columns"] with a compare op, the value's `kind` (abi.KIND_*) and the value
    (an int for the integer kinds and Bool, a float for the float kinds, bytes as stored
    otherwise), or with op "present" / "absent"; or the `status` tensor of header_columns()
    (no op: true where the headers are valid)."""
    import struct

    from . import abi
    if isinstance(source, str):
        width = 16 if source == "id" else 8
        return abi.SelectClause.make(_SEL_SOURCES[source], _SEL_OPS[op],
                                     (int(value) % (1 << (8 * width))).to_bytes(width, "little"))
    if not isinstance(source, dict):
        return abi.SelectClause.make(abi.SEL_HEADER_STATUS, status=source.data_ptr())
    col = abi.HeaderColumn(source["value_kinds"].data_ptr(), source["value_lengths"].data_ptr(), None,
                           source["values16"].data_ptr())
    if op in ("present", "absent"):
        return abi.SelectClause.make(abi.SEL_HEADER, _SEL_OPS[op], column=col)
    if isinstance(value, float):
        value = struct.pack("<f" if kind == abi.KIND_FLOAT32 else "<d", value)
    elif isinstance(value, int):
        size = _SEL_KIND_SIZE[kind]
        value = (value % (1 << (8 * size))).to_bytes(size, "little")
    return abi.SelectClause.make(abi.SEL_HEADER, _SEL_OPS[op], bytes(value), kind, col)


def select_messages(cx, arrays: dict, clauses=(), mask=None, cursor=None) -> dict:
    """Keep the messages of `arrays` (the dict unpack_record returns) that pass every clause
    (select_clause(...) or abi.SelectClause objects, at most 8) and whose `mask` entry (an
    optional uint8 CUDA tensor of `count`) is nonzero, compacted in source order
    (iggy_codec_select_messages_device): enqueued on the current stream with the stream
    handling of unpack_record, then ONE synchronise.

    Outputs are allocated at the source's capacities. Returns the arrays of unpack_record
    trimmed to the kept `count`, plus `source_index` [count] (int64: which source message each
    kept one was, to gather header columns or other per-message tensors), `first_message`,
    `examined`, and `raw`, an abi.RawMessages of the kept messages for Codec.encode_device.

    cursor: as unpack_record's (an int64 CUDA tensor of 4 that this call advances), so that
    selects and unpacks append into one numbering; the returned tensors are this call's part.
    Raises CodecError carrying the wire error of a failed select."""
    import ctypes

    import torch

    from . import abi
    from .codec import CodecError

    n = int(arrays["count"])
    dev = arrays["payloads"].device
    names = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
             "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")
    for k in names:
        if not arrays[k].is_cuda or not arrays[k].is_contiguous():
            raise ValueError(f"arrays[{k!r}] must be a contiguous CUDA tensor")
    sp, su = int(arrays.get("payload_base", 0)), int(arrays.get("user_headers_base", 0))
    np_, nu = arrays["payloads"].numel(), arrays["user_headers"].numel()
    # (the starts are absolute positions: the byte arrays' bases are their positions 0)
    # (an empty byte array has no address: it is left out of the source and of the output)
    empty = {k for k in ("payloads", "user_headers") if arrays[k].numel() == 0}
    src = abi.UnpackedMessages(n, sp + np_, su + nu, *(
        None if k in empty else arrays[k].data_ptr() - (sp if k == "payloads" else su if k == "user_headers" else 0)
        for k in names))
    bm = bp = bu = 0
    if cursor is not None:
        bm, bp, bu = (int(x) for x in to_host(cursor)[:3])

    def arr(k, dtype):
        return torch.empty(max(k, 1), dtype=dtype, device=dev)

    i64 = torch.int64
    t = {
        "ids": arr(2 * (bm + n), i64), "checksums": arr(bm + n, i64), "offsets": arr(bm + n, i64),
        "timestamps": arr(bm + n, i64), "origin_timestamps": arr(bm + n, i64),
        "payload_lengths": arr(bm + n, torch.int32), "user_headers_lengths": arr(bm + n, torch.int32),
        "payload_starts": arr(bm + n + 1, i64), "user_headers_starts": arr(bm + n + 1, i64),
        "payloads": arr(bp + np_, torch.uint8), "user_headers": arr(bu + nu, torch.uint8),
    }
    out = abi.UnpackedMessages(bm + n, bp + np_, bu + nu, *(None if k in empty else t[k].data_ptr() for k in names))
    d_idx = arr(bm + n, i64)
    d_cnt = to_device(np.array([n], dtype=np.int64), dev)
    d_res = torch.zeros(ctypes.sizeof(abi.SelectResult), dtype=torch.uint8, device=dev)
    spec = abi.SelectSpec.make(list(clauses), mask.data_ptr() if mask is not None else None)
    cur = torch.cuda.current_stream(dev)  # (stream handling as unpack_record)
    work = cur if cur.cuda_stream else torch.cuda.ExternalStream(cx.stream(), device=dev)
    if work is not cur:
        work.wait_stream(cur)
    rc = cx.select_messages_device(src, d_cnt.data_ptr(), spec, out, d_idx.data_ptr(),
                                   cursor.data_ptr() if cursor is not None else None, d_res.data_ptr(),
                                   work.cuda_stream)
    if rc:
        raise CodecError(rc, None, "select_messages")
    if work is not cur:
        cur.wait_stream(work)
    res = abi.SelectResult.from_buffer_copy(to_host(d_res).tobytes())  # the one synchronise
    if res.error.kind != abi.OK:
        raise CodecError(res.error.kind, res.error, "select_messages")
    c, f = res.count, res.first_message
    r = {k: t[k][f:f + c] for k in ("checksums", "offsets", "timestamps", "origin_timestamps",
                                    "payload_lengths", "user_headers_lengths")}
    r["ids"] = t["ids"][2 * f:2 * (f + c)].view(c, 2)
    r["payload_starts"] = t["payload_starts"][f:f + c + 1]
    r["user_headers_starts"] = t["user_headers_starts"][f:f + c + 1]
    r["payloads"] = t["payloads"][bp:bp + res.payload_bytes]
    r["user_headers"] = t["user_headers"][bu:bu + res.user_headers_bytes]
    r["source_index"] = d_idx[f:f + c]
    r["count"], r["first_message"], r["examined"] = c, f, res.examined
    r["payload_base"], r["user_headers_base"] = bp, bu
    r["raw"] = abi.RawMessages(c, r["ids"].data_ptr(), r["origin_timestamps"].data_ptr(), r["payloads"].data_ptr(),
                               r["payload_lengths"].data_ptr(),
                               r["user_headers"].data_ptr() if res.user_headers_bytes else None,
                               r["user_headers_lengths"].data_ptr())
    if c and res.min_payload_length == res.max_payload_length:
        r["payloads_2d"] = r["payloads"].view(c, res.max_payload_length)
    return r


def route_messages(cx, arrays: dict, partitions: int, key="id", mask=None, absent=None) -> dict:
    """Route the messages of `arrays` (the dict unpack_record, select_messages or this
    function returns) to `partitions` (1..256) partitions by the reference's rule,
    XXH32(key) % partitions, and group them per partition, stable inside a partition
    (iggy_codec_route_messages_device): enqueued on the current stream with the stream
    handling of unpack_record, then ONE synchronise.

    key: "id" (the 16 id bytes, messages_key_u128(id)); ("header", column) with one column
    dict of header_columns()["columns"] (the whole stored value is the key; a message without
    it goes to partition `absent`, or is dropped when `absent` is None); ("bytes", tensor)
    with a [count, L] uint8 CUDA tensor of fixed-length keys, L in 1..255 (its row stride is
    the key stride); ("partition", tensor) with an int32 CUDA tensor of partition indices,
    used as they are (>= partitions: dropped). mask: an optional uint8 CUDA tensor of `count`;
    a message whose entry is zero is dropped.

    Returns the arrays of unpack_record holding the routed `count` messages ordered by
    (partition, source index), plus `partition_first`, `partition_payload_first`,
    `partition_user_headers_first` (host lists of partitions + 1), `partition_of` [examined]
    (int32 CUDA tensor, -1 = dropped), `source_index` [count], `examined`, `dropped`,
    `partitions`, and `raw(p)`, the abi.RawMessages of partition p for Codec.encode_device.
    Raises CodecError carrying the wire error of a failed route."""
    import ctypes

    import torch

    from . import abi
    from .codec import CodecError

    n = int(arrays["count"])
    dev = arrays["payloads"].device
    names = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
             "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")
    for k in names:
        if not arrays[k].is_cuda or not arrays[k].is_contiguous():
            raise ValueError(f"arrays[{k!r}] must be a contiguous CUDA tensor")
    sp, su = int(arrays.get("payload_base", 0)), int(arrays.get("user_headers_base", 0))
    np_, nu = arrays["payloads"].numel(), arrays["user_headers"].numel()
    # (as select_messages: the starts are absolute, an empty byte array is left out)
    empty = {k for k in ("payloads", "user_headers") if arrays[k].numel() == 0}
    src = abi.UnpackedMessages(n, sp + np_, su + nu, *(
        None if k in empty else arrays[k].data_ptr() - (sp if k == "payloads" else su if k == "user_headers" else 0)
        for k in names))
    d_mask = mask.data_ptr() if mask is not None else None
    drop = abi.ROUTE_DROP if absent is None else int(absent)
    keep = None  # (tensors the spec points at)
    if key == "id":
        spec = abi.RouteSpec.make(partitions, abi.ROUTE_KEY_ID, mask=d_mask)
    elif key[0] == "header":
        col = key[1]
        if "user_headers" in empty:  # no header bytes at all: every key is absent, nothing is read
            keep = torch.zeros(16, dtype=torch.uint8, device=dev)
            src.user_headers = keep.data_ptr()
        spec = abi.RouteSpec.make(partitions, abi.ROUTE_KEY_HEADER, drop, mask=d_mask, column=abi.HeaderColumn(
            col["value_kinds"].data_ptr(), col["value_lengths"].data_ptr(), col["value_pos"].data_ptr(), None))
    elif key[0] == "bytes":
        keep = key[1]
        if keep.dtype != torch.uint8 or keep.dim() != 2 or keep.stride(1) != 1 or keep.shape[0] < n:
            raise ValueError("bytes keys must be a [count, L] uint8 CUDA tensor with unit inner stride")
        spec = abi.RouteSpec.make(partitions, abi.ROUTE_KEY_BYTES, keys=keep.data_ptr(), key_length=keep.shape[1],
                                  key_stride=keep.stride(0), mask=d_mask)
    elif key[0] == "partition":
        keep = key[1]
        if keep.dtype != torch.int32 or not keep.is_contiguous() or keep.numel() < n:
            raise ValueError("partition ids must be a contiguous int32 CUDA tensor of count")
        spec = abi.RouteSpec.make(partitions, abi.ROUTE_KEY_PARTITION, partition_ids=keep.data_ptr(), mask=d_mask)
    else:
        raise ValueError("key must be 'id', ('header', column), ('bytes', tensor) or ('partition', tensor)")

    def arr(k, dtype):
        return torch.empty(max(k, 1), dtype=dtype, device=dev)

    i64 = torch.int64
    t = {
        "ids": arr(2 * n, i64), "checksums": arr(n, i64), "offsets": arr(n, i64), "timestamps": arr(n, i64),
        "origin_timestamps": arr(n, i64), "payload_lengths": arr(n, torch.int32),
        "user_headers_lengths": arr(n, torch.int32), "payload_starts": arr(n + 1, i64),
        "user_headers_starts": arr(n + 1, i64), "payloads": arr(np_, torch.uint8), "user_headers": arr(nu, torch.uint8),
    }
    out = abi.UnpackedMessages(n, np_, nu, *(None if k in empty else t[k].data_ptr() for k in names))
    npart = max(int(partitions), 0) + 1
    d_tab = torch.zeros((3, npart), dtype=i64, device=dev)  # first, payload first, user-headers first
    d_of, d_idx = arr(n, torch.int32), arr(n, i64)
    d_cnt = to_device(np.array([n], dtype=np.int64), dev)
    d_res = torch.zeros(ctypes.sizeof(abi.RouteResult), dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev)  # (stream handling as unpack_record)
    work = cur if cur.cuda_stream else torch.cuda.ExternalStream(cx.stream(), device=dev)
    if work is not cur:
        work.wait_stream(cur)
    rc = cx.route_messages_device(src, d_cnt.data_ptr(), spec, out, d_tab[0].data_ptr(), d_tab[1].data_ptr(),
                                  d_tab[2].data_ptr(), d_of.data_ptr(), d_idx.data_ptr(), d_res.data_ptr(),
                                  work.cuda_stream)
    if rc:
        raise CodecError(rc, None, "route_messages")
    if work is not cur:
        cur.wait_stream(work)
    # the result and the three tables in one copy: the one synchronise
    back = to_host(torch.cat([d_res, d_tab.view(torch.uint8).reshape(-1)]))
    res = abi.RouteResult.from_buffer_copy(back[:d_res.numel()].tobytes())
    if res.error.kind != abi.OK:
        raise CodecError(res.error.kind, res.error, "route_messages")
    tab = back[d_res.numel():].view(np.int64).reshape(3, npart)
    c = res.count
    r = {k: t[k][:c] for k in ("checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
                               "user_headers_lengths")}
    r["ids"] = t["ids"][:2 * c].view(c, 2)
    r["payload_starts"], r["user_headers_starts"] = t["payload_starts"][:c + 1], t["user_headers_starts"][:c + 1]
    r["payloads"], r["user_headers"] = t["payloads"][:res.payload_bytes], t["user_headers"][:res.user_headers_bytes]
    r["source_index"], r["partition_of"] = d_idx[:c], d_of[:n]
    r["count"], r["examined"], r["dropped"], r["partitions"] = c, res.examined, res.dropped, res.partitions
    r["first_message"], r["payload_base"], r["user_headers_base"] = 0, 0, 0
    first, pfirst, ufirst = (tab[k].tolist() for k in range(3))
    if "payloads" in empty:
        pfirst = [0] * npart
    if "user_headers" in empty:
        ufirst = [0] * npart
    r["partition_first"], r["partition_payload_first"], r["partition_user_headers_first"] = first, pfirst, ufirst

    def raw(p: int):
        """The abi.RawMessages of partition p (offset pointers into the routed arrays)."""
        a, b = first[p], first[p + 1]
        uh = res.user_headers_bytes and ufirst[p + 1] > ufirst[p]
        return abi.RawMessages(b - a, t["ids"].data_ptr() + 16 * a, t["origin_timestamps"].data_ptr() + 8 * a,
                               t["payloads"].data_ptr() + pfirst[p], t["payload_lengths"].data_ptr() + 4 * a,
                               t["user_headers"].data_ptr() + ufirst[p] if uh else None,
                               t["user_headers_lengths"].data_ptr() + 4 * a)

    r["raw"] = raw
    return r


def to_host(t) -> np.ndarray:
    """A numpy copy of tensor `t` (synchronous; the copy lands in pinned memory)."""
    import torch
    if t.device.type == "cpu":
        return t.numpy()
    if _PAGEABLE:
        return t.cpu().numpy()
    p = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    p.copy_(t)
    return p.numpy()
