"""Plain numpy / Python restatement of the device select (include/iggy_codec.h "select"),
the expected values of the select tests (never the code under test; it does not import the
library): the truth of a clause for one message, the refusals of a malformed spec, and the
stable compaction of every array with the cursor's bases.

A source is a dict of numpy arrays shaped like iggy_unpacked_messages: ids [2n] u64,
checksums / offsets / timestamps / origin_timestamps [n] u64, payload_lengths /
user_headers_lengths [n] u32, payload_starts / user_headers_starts [n + 1] u64, payloads /
user_headers u8 (a missing key = a NULL array).
A clause is a Clause tuple; a header column is a dict of value_kinds [n] u8, value_lengths
[n] u8 and values16 [n, 16] u8; a status array is [n, 4] u32 (kind first)."""
import math
import struct
from collections import namedtuple

import numpy as np

(SEL_OFFSET, SEL_TIMESTAMP, SEL_ORIGIN_TIMESTAMP, SEL_PAYLOAD_LENGTH, SEL_USER_HEADERS_LENGTH, SEL_ID, SEL_HEADER,
 SEL_HEADER_STATUS) = range(1, 9)
(OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE, OP_PRESENT, OP_ABSENT) = range(1, 9)
COMPARE_OPS = (OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE)
ORDER_OPS = (OP_LT, OP_LE, OP_GT, OP_GE)
(K_RAW, K_STRING, K_BOOL, K_INT8, K_INT16, K_INT32, K_INT64, K_INT128, K_UINT8, K_UINT16, K_UINT32, K_UINT64,
 K_UINT128, K_FLOAT32, K_FLOAT64) = range(1, 16)
KIND_SIZE = {K_BOOL: 1, K_INT8: 1, K_INT16: 2, K_INT32: 4, K_INT64: 8, K_INT128: 16, K_UINT8: 1, K_UINT16: 2,
             K_UINT32: 4, K_UINT64: 8, K_UINT128: 16, K_FLOAT32: 4, K_FLOAT64: 8}
SIGNED = (K_INT8, K_INT16, K_INT32, K_INT64, K_INT128)
ERR_INVALID_ARGUMENT = 101
ERR_CAPACITY = 102

U64_SOURCES = {SEL_OFFSET: "offsets", SEL_TIMESTAMP: "timestamps", SEL_ORIGIN_TIMESTAMP: "origin_timestamps"}
U32_SOURCES = {SEL_PAYLOAD_LENGTH: "payload_lengths", SEL_USER_HEADERS_LENGTH: "user_headers_lengths"}
FIXED = ("checksums", "offsets", "timestamps", "origin_timestamps")

Clause = namedtuple("Clause", "source op kind length operand column status", defaults=(0, 0, 0, b"", None, None))


def clause(source, op=0, operand=b"", kind=0, column=None, status=None, length=None):
    operand = bytes(operand)
    return Clause(source, op, kind, len(operand) if length is None else length, operand, column, status)


def _op(op, a, b):
    return {OP_EQ: a == b, OP_NE: a != b, OP_LT: a < b, OP_LE: a <= b, OP_GT: a > b, OP_GE: a >= b}[op]


def refused(clauses, src) -> bool:
    """True when both entry points refuse the spec synchronously (IGGY_ERR_INVALID_ARGUMENT)."""
    if len(clauses) > 8:
        return True
    for c in clauses:
        if c.source in U64_SOURCES or c.source in U32_SOURCES or c.source == SEL_ID:
            name = U64_SOURCES.get(c.source) or U32_SOURCES.get(c.source) or "ids"
            if c.op not in COMPARE_OPS or src.get(name) is None:
                return True
        elif c.source == SEL_HEADER_STATUS:
            if c.status is None:
                return True
        elif c.source == SEL_HEADER:
            col = c.column or {}
            if col.get("value_kinds") is None:
                return True
            if c.op in (OP_PRESENT, OP_ABSENT):
                continue
            if c.op not in COMPARE_OPS or not 1 <= c.kind <= 15 or col.get("values16") is None:
                return True
            if c.kind in KIND_SIZE:
                if c.length != KIND_SIZE[c.kind]:
                    return True
            elif not 1 <= c.length <= 16 or col.get("value_lengths") is None:
                return True
            if c.kind in (K_RAW, K_STRING, K_BOOL) and c.op in ORDER_OPS:
                return True
        else:
            return True
    return False


def _typed(kind, b):
    """The value of `kind` stored little-endian in bytes b (its fixed size); None for a NaN."""
    if kind == K_FLOAT32:
        v = struct.unpack("<f", b)[0]
        return None if math.isnan(v) else v
    if kind == K_FLOAT64:
        v = struct.unpack("<d", b)[0]
        return None if math.isnan(v) else v
    return int.from_bytes(b, "little", signed=kind in SIGNED)


def clause_true(c, src, i) -> bool:
    if c.source in U64_SOURCES:
        return _op(c.op, int(src[U64_SOURCES[c.source]][i]), int.from_bytes((c.operand + bytes(16))[:8], "little"))
    if c.source in U32_SOURCES:
        return _op(c.op, int(src[U32_SOURCES[c.source]][i]), int.from_bytes((c.operand + bytes(16))[:4], "little"))
    if c.source == SEL_ID:
        v = int(src["ids"][2 * i]) | (int(src["ids"][2 * i + 1]) << 64)
        return _op(c.op, v, int.from_bytes((c.operand + bytes(16))[:16], "little"))
    if c.source == SEL_HEADER_STATUS:
        return int(np.asarray(c.status).reshape(-1, 4)[i, 0]) == 0
    k = int(c.column["value_kinds"][i])
    if c.op == OP_PRESENT:
        return k != 0
    if c.op == OP_ABSENT:
        return k == 0
    if k != c.kind:
        return False  # absent or another kind: false under every compare op, NE included
    stored = bytes(np.asarray(c.column["values16"]).reshape(-1, 16)[i])
    operand = (c.operand + bytes(16))[:c.length]
    if k in (K_RAW, K_STRING):
        eq = int(c.column["value_lengths"][i]) == c.length and stored[:c.length] == operand
        return eq if c.op == OP_EQ else not eq
    a, b = _typed(k, stored[:c.length]), _typed(k, operand)
    if a is None or b is None:
        return c.op == OP_NE  # a NaN on either side
    return _op(c.op, a, b)


def keep_mask(src, count, clauses, mask=None) -> np.ndarray:
    keep = np.zeros(count, dtype=bool)
    for i in range(count):
        keep[i] = (mask is None or mask[i] != 0) and all(clause_true(c, src, i) for c in clauses)
    return keep


def lengths(src, what, count) -> np.ndarray:
    """payload ("payload") or user-header ("user_headers") lengths as the select takes them."""
    if src.get(f"{what}_lengths") is not None:
        return np.asarray(src[f"{what}_lengths"][:count], dtype=np.uint64)
    if src.get(f"{what}_starts") is not None:
        return np.diff(np.asarray(src[f"{what}_starts"][:count + 1], dtype=np.uint64)).astype(np.uint64)
    return np.zeros(count, dtype=np.uint64)


def compact(src, count, keep, first=0, base_pl=0, base_uh=0) -> dict:
    """The stable compaction of every array of src for the keep verdicts: the kept part of
    each output array (the starts absolute, with the end entry), the source index, and the
    result fields (count, payload_bytes, user_headers_bytes, first_message, min / max)."""
    idx = np.flatnonzero(keep[:count]).astype(np.uint64)
    pl, uh = lengths(src, "payload", count)[idx.astype(np.int64)], lengths(src, "user_headers", count)[idx.astype(np.int64)]
    out = {"source_index": idx, "count": int(idx.size), "first_message": first,
           "payload_bytes": int(pl.sum()), "user_headers_bytes": int(uh.sum()),
           "min_payload_length": int(pl.min()) if idx.size else 0,
           "max_payload_length": int(pl.max()) if idx.size else 0,
           "payload_lengths": pl.astype(np.uint32), "user_headers_lengths": uh.astype(np.uint32),
           "payload_starts": (np.concatenate([[0], np.cumsum(pl)]).astype(np.uint64) + np.uint64(base_pl)),
           "user_headers_starts": (np.concatenate([[0], np.cumsum(uh)]).astype(np.uint64) + np.uint64(base_uh))}
    ii = idx.astype(np.int64)
    for k in FIXED:
        if src.get(k) is not None:
            out[k] = np.asarray(src[k])[ii]
    if src.get("ids") is not None:
        out["ids"] = np.asarray(src["ids"]).reshape(-1, 2)[ii].reshape(-1)
    for what, name, ln in (("payload", "payloads", pl), ("user_headers", "user_headers", uh)):
        if src.get(name) is not None and src.get(f"{what}_starts") is not None:
            st = np.asarray(src[f"{what}_starts"])
            parts = [np.asarray(src[name])[int(st[i]):int(st[i]) + int(l)] for i, l in zip(ii, ln)]
            out[name] = np.concatenate(parts + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return out


def select(src, count, clauses, mask=None, first=0, base_pl=0, base_uh=0) -> dict:
    return compact(src, count, keep_mask(src, count, clauses, mask), first, base_pl, base_uh)
