"""Plain numpy / Python restatement of the device route (include/iggy_codec.h "route"), the
expected values of the route tests (never the code under test; it does not import the
library): its own XXH32 (from the published specification, pinned by
tests/golden/xxh32_vectors.json), the partition rule, the drop rules, the refusals of a
malformed spec, and the stable (partition, source index) order of every array with the
three tables.

A source is a dict of numpy arrays as in tests/select_ref.py. A spec is a Spec tuple:
`keys` a [n, stride] u8 array for BYTES, `partition_ids` a [n] u32 array for PARTITION,
`column` a dict of value_kinds / value_lengths [n] u8 and value_pos [n] u32 for HEADER."""
from collections import namedtuple

import numpy as np

import select_ref as S

(KEY_ID, KEY_HEADER, KEY_BYTES, KEY_PARTITION) = range(1, 5)
DROP = 0xFFFFFFFF
MAX_PARTITIONS = 256
ERR_INVALID_ARGUMENT = S.ERR_INVALID_ARGUMENT
ERR_CAPACITY = S.ERR_CAPACITY

P1, P2, P3, P4, P5 = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1
M = 0xFFFFFFFF

Spec = namedtuple("Spec", "partitions key_source absent key_length key_stride keys partition_ids column mask",
                  defaults=(DROP, 0, 0, None, None, None, None))


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def _round(acc, word):
    return (_rotl((acc + word * P2) & M, 13) * P1) & M


def xxh32(data, seed=0) -> int:
    data = bytes(data)
    n, at = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed & M, (seed - P1) & M]
        while at + 16 <= n:
            for k in range(4):
                v[k] = _round(v[k], int.from_bytes(data[at + 4 * k:at + 4 * k + 4], "little"))
            at += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while at + 4 <= n:
        h = (_rotl((h + int.from_bytes(data[at:at + 4], "little") * P3) & M, 17) * P4) & M
        at += 4
    while at < n:
        h = (_rotl((h + data[at] * P5) & M, 11) * P1) & M
        at += 1
    h ^= h >> 15
    h = (h * P2) & M
    h ^= h >> 13
    h = (h * P3) & M
    return h ^ (h >> 16)


def refused(spec, src) -> bool:
    """True when both entry points refuse the spec synchronously (IGGY_ERR_INVALID_ARGUMENT)."""
    if not 1 <= spec.partitions <= MAX_PARTITIONS:
        return True
    if spec.absent != DROP and spec.absent >= spec.partitions:
        return True
    if spec.key_source == KEY_ID:
        return src.get("ids") is None
    if spec.key_source == KEY_HEADER:
        col = spec.column or {}
        return (any(col.get(k) is None for k in ("value_kinds", "value_lengths", "value_pos"))
                or src.get("user_headers_starts") is None or src.get("user_headers") is None)
    if spec.key_source == KEY_BYTES:
        return spec.keys is None or not 1 <= spec.key_length <= 255 or spec.key_stride < spec.key_length
    if spec.key_source == KEY_PARTITION:
        return spec.partition_ids is None
    return True


def key_of(spec, src, i):
    """The key bytes of message i, None when it has none (HEADER: absent), for the hashed sources."""
    if spec.key_source == KEY_ID:
        return int(src["ids"][2 * i]).to_bytes(8, "little") + int(src["ids"][2 * i + 1]).to_bytes(8, "little")
    if spec.key_source == KEY_BYTES:
        flat = np.asarray(spec.keys).reshape(-1)
        return bytes(flat[i * spec.key_stride:i * spec.key_stride + spec.key_length])
    b, e = int(src["user_headers_starts"][i]), int(src["user_headers_starts"][i + 1])
    at, ln = int(spec.column["value_pos"][i]), int(spec.column["value_lengths"][i])
    if int(spec.column["value_kinds"][i]) == 0 or ln == 0 or at + ln > e - b:
        return None
    return bytes(src["user_headers"][b + at:b + at + ln])


def partitions_of(spec, src, count) -> np.ndarray:
    """[count] u32: the partition of every message, DROP for a dropped one."""
    out = np.full(count, DROP, dtype=np.uint32)
    for i in range(count):
        if spec.mask is not None and spec.mask[i] == 0:
            continue
        if spec.key_source == KEY_PARTITION:
            v = int(spec.partition_ids[i])
            out[i] = v if v < spec.partitions else DROP
            continue
        key = key_of(spec, src, i)
        out[i] = spec.absent if key is None else xxh32(key) % spec.partitions
    return out


def route(spec, src, count) -> dict:
    """The routed arrays in (partition, source index) order (select_ref.compact's fields of
    the stable order), partition_of, and the three [partitions + 1] tables."""
    part = partitions_of(spec, src, count)
    order = np.concatenate([np.flatnonzero(part == p) for p in range(spec.partitions)] +
                           [np.zeros(0, np.int64)]).astype(np.int64)
    pl, uh = S.lengths(src, "payload", count)[order], S.lengths(src, "user_headers", count)[order]
    out = {"partition_of": part, "source_index": order.astype(np.uint64), "count": int(order.size),
           "dropped": count - int(order.size), "payload_bytes": int(pl.sum()), "user_headers_bytes": int(uh.sum()),
           "payload_lengths": pl.astype(np.uint32), "user_headers_lengths": uh.astype(np.uint32),
           "payload_starts": np.concatenate([[0], np.cumsum(pl)]).astype(np.uint64),
           "user_headers_starts": np.concatenate([[0], np.cumsum(uh)]).astype(np.uint64)}
    counts = np.array([int((part == p).sum()) for p in range(spec.partitions)], dtype=np.uint64)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    out["partition_first"] = first
    out["partition_payload_first"] = out["payload_starts"][first.astype(np.int64)]
    out["partition_user_headers_first"] = out["user_headers_starts"][first.astype(np.int64)]
    for k in S.FIXED:
        if src.get(k) is not None:
            out[k] = np.asarray(src[k])[order]
    if src.get("ids") is not None:
        out["ids"] = np.asarray(src["ids"]).reshape(-1, 2)[order].reshape(-1)
    for what, name, ln in (("payload", "payloads", pl), ("user_headers", "user_headers", uh)):
        if src.get(name) is not None and src.get(f"{what}_starts") is not None:
            st = np.asarray(src[f"{what}_starts"])
            parts = [np.asarray(src[name])[int(st[i]):int(st[i]) + int(l)] for i, l in zip(order, ln)]
            out[name] = np.concatenate(parts + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return out
