"""GPU tests of the device route (iggy_codec_route_messages_device, route.hip): the partition
of every message by XXH32(key) % partitions, then the stable (partition, source index)
split of the routed messages into a second set of arrays with its three tables.

Expected values come from the plain numpy restatement (tests/route_ref.py) alone. Inputs
are numpy arrays put on the device with torch_io.to_device. Every output array, every
table, partition_of and source_index sit between 0xA5 guards that must survive every call,
errors included; what lies past the routed part of an array must stay 0xA5 too. Integer
byte work: every comparison is bit-exact."""
import ctypes

import numpy as np
import pytest

import route_ref as R
import route_util as RU
import select_ref as SR
import select_util as U
from iggy_amd import abi
from iggy_amd.torch_io import to_device, to_host

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
TILE = 2048  # source messages per tile of route.hip
FIELDS = U.FIELDS
U64 = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_starts", "user_headers_starts",
       "source_index", "partition_first", "partition_payload_first", "partition_user_headers_first")
U32 = ("payload_lengths", "user_headers_lengths", "partition_of")
BYTES = ("payloads", "user_headers")
TABLES = ("partition_first", "partition_payload_first", "partition_user_headers_first")
EXTRA = TABLES + ("partition_of", "source_index")
BAD = abi.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def cx():
    from iggy_amd.codec import Codec
    c = Codec(0)
    yield c
    c.close()


# ------------------------------------------------------------------ harness
class Dev:
    """Host arrays on the device, one tensor each (kept alive); ptr(a) -> its device address.
    shift: the payloads / user_headers arrays start `shift` bytes into their tensors; shifts:
    id(array) -> the same for any other array (a BYTES key array)."""

    def __init__(self, shift=0, shifts=None):
        self.t, self.shift, self.shifts = {}, shift, shifts or {}

    def ptr(self, a, byte_array=False):
        key = id(a)
        if key not in self.t:
            flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            sh = self.shift if byte_array else self.shifts.get(key, 0)
            buf = np.zeros(max(flat.size + sh, 1), np.uint8)
            buf[sh:sh + flat.size] = flat
            self.t[key] = (to_device(buf, "cuda:0"), sh, a)
        t, sh, _ = self.t[key]
        return t.data_ptr() + sh

    def source(self, src, cap, cap_p=None, cap_u=None):
        bytes_ids = {id(src[k]) for k in BYTES if src.get(k) is not None}
        return U.src_struct(src, cap, lambda a: self.ptr(a, id(a) in bytes_ids), cap_p, cap_u)


class Outs:
    """Every output array, the three tables, partition_of and the source index as
    [front guard | capacity | back guard] of 0xA5."""

    def __init__(self, cap_m, cap_p, cap_u, partitions, cap_src, shift=0, skip=()):
        import torch
        self.cap = (cap_m, cap_p, cap_u)
        self.t, self.front, self.size = {}, {}, {}
        for k in FIELDS + EXTRA:
            if k in skip:
                continue
            front = GUARD
            if k in BYTES:
                size, front = (cap_p if k == "payloads" else cap_u), GUARD + shift
            elif k in TABLES:
                size = 8 * (partitions + 1)
            elif k == "partition_of":
                size = 4 * cap_src
            elif k in U32:
                size = 4 * cap_m
            elif k == "ids":
                size = 16 * cap_m
            elif k.endswith("_starts"):
                size = 8 * (cap_m + 1)
            else:
                size = 8 * cap_m
            self.t[k] = torch.full((front + size + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
            self.front[k], self.size[k] = front, size

    def ptr(self, k):
        return self.t[k].data_ptr() + self.front[k] if k in self.t else None

    def struct(self):
        return abi.UnpackedMessages(*self.cap, *(self.ptr(k) for k in FIELDS))

    def host(self):
        """-> {field: typed numpy view of the capacity region}; asserts the guards."""
        out = {}
        for k, t in self.t.items():
            h = to_host(t)
            f, s = self.front[k], self.size[k]
            assert (h[:f] == FILL).all(), f"front guard of {k}"
            assert (h[f + s:] == FILL).all(), f"back guard of {k}"
            body = h[f:f + s].copy()
            out[k] = body.view(np.uint64) if k in U64 else body.view(np.uint32) if k in U32 else body
        return out

    def untouched(self, but=()):
        return all((to_host(t) == FILL).all() for k, t in self.t.items() if k not in but)


def _enqueue(cx, dev, src, count, spec, outs, cap=None, cap_p=None, cap_u=None, hash_only=False, d_count=None):
    """One route on the current stream, no synchronise -> (result tensor, keep-alive)."""
    import torch
    s = dev.source(src, count if cap is None else cap, cap_p, cap_u)
    q = RU.abi_spec(spec, dev.ptr)
    d_cnt = to_device(np.array([count], dtype=np.int64), "cuda:0")
    d_res = torch.full((ctypes.sizeof(abi.RouteResult),), 0xEE, dtype=torch.uint8, device="cuda:0")
    rc = cx.route_messages_device(s, d_cnt.data_ptr() if d_count is None else d_count, q,
                                  None if hash_only else outs.struct(), outs.ptr("partition_first"),
                                  outs.ptr("partition_payload_first"), outs.ptr("partition_user_headers_first"),
                                  outs.ptr("partition_of"), outs.ptr("source_index"), d_res.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return d_res, (d_cnt, s, q)


def _result(d_res):
    return abi.RouteResult.from_buffer_copy(to_host(d_res).tobytes())


def _check(got, x, n, partitions):
    """Every array the call wrote against the restatement; what lies past it stays 0xA5."""
    c = x["count"]
    fill64, fill32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)
    for k in ("checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths", "user_headers_lengths",
              "source_index"):
        if k in got and k in x:
            assert np.array_equal(got[k][:c], x[k]), k
            assert (got[k][c:] == (fill32 if k in U32 else fill64)).all(), k
    if "ids" in got:
        assert np.array_equal(got["ids"][:2 * c], x["ids"]) and (got["ids"][2 * c:] == fill64).all()
    for k in ("payload_starts", "user_headers_starts"):
        if k in got:
            assert np.array_equal(got[k][:c + 1], x[k]), k
            assert (got[k][c + 1:] == fill64).all(), k
    for k in BYTES:
        if k in got:
            assert np.array_equal(got[k][:x[k].size], x[k]), k
            assert (got[k][x[k].size:] == FILL).all(), k
    if "partition_of" in got:
        assert np.array_equal(got["partition_of"][:n], x["partition_of"])
        assert (got["partition_of"][n:] == fill32).all()
    for k in TABLES:
        if k in got:
            assert got[k].size == partitions + 1 and np.array_equal(got[k], x[k]), k


def _check_result(res, x, n, partitions):
    assert res.error.astuple() == (0, 0, 0, 0, 0), res.error
    assert (res.examined, res.count, res.dropped, res.payload_bytes, res.user_headers_bytes, res.partitions) == \
        (n, x["count"], x["dropped"], x["payload_bytes"], x["user_headers_bytes"], partitions)
    assert res.count + res.dropped == res.examined


def _count(src):
    return src["payload_lengths"].size if src.get("payload_lengths") is not None else src["payload_starts"].size - 1


def _route_and_check(cx, src, spec, src_shift=0, out_shift=0, slack=0, skip=(), exact=True, shifts=None, x=None):
    """The route of `src` by `spec` against the restatement, at capacities of exactly what is
    routed (exact) or the source's sizes plus slack."""
    import torch
    n = _count(src)
    x = R.route(spec, src, n) if x is None else x
    pb = src["payloads"].size if src.get("payloads") is not None else 0
    ub = src["user_headers"].size if src.get("user_headers") is not None else 0
    if exact:
        outs = Outs(x["count"], x["payload_bytes"], x["user_headers_bytes"], spec.partitions, n, out_shift, skip)
    else:
        outs = Outs(n + slack, pb + slack, ub + slack, spec.partitions, n + slack, out_shift, skip)
    dev = Dev(src_shift, shifts)
    d_res, keepalive = _enqueue(cx, dev, src, n, spec, outs, cap=None if exact else n + slack)
    torch.cuda.synchronize()
    res = _result(d_res)
    _check_result(res, x, n, spec.partitions)
    got = outs.host()
    _check(got, x, n, spec.partitions)
    return res, got, x


def _source(n, seed=1):
    return U.make_source(np.arange(n) % 23, np.where(np.arange(n) % 3 == 0, 5, 0), seed)


def _by_ids(partitions, ids, mask=None):
    return R.Spec(partitions, R.KEY_PARTITION, partition_ids=np.asarray(ids, dtype=np.uint32), mask=mask)


# ------------------------------------------------------------------ counts
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_counts(cx, n):
    src = _source(n, seed=n + 1)
    _, _, x = _route_and_check(cx, src, R.Spec(3, R.KEY_ID), exact=False, slack=2)
    assert x["dropped"] == 0
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    _, _, x = _route_and_check(cx, src, R.Spec(3, R.KEY_ID, mask=mask))  # the mask
    assert x["dropped"] == int((mask == 0).sum()) and np.array_equal(x["partition_of"] == R.DROP, mask == 0)


def test_a_table_of_many_tiles_and_256_partitions(cx):
    """70 000 messages of 0..40 B into 256 partitions: every thread of the scan's workgroup
    walks 35 rows of the [tile][partition] table."""
    rng = np.random.default_rng(70)
    src = U.make_source(rng.integers(0, 41, size=70_000), seed=70)
    ids = rng.integers(0, 260, size=70_000)  # (four values drop)
    _, _, x = _route_and_check(cx, src, _by_ids(256, ids))
    assert x["dropped"] > 0 and (np.diff(x["partition_first"].astype(np.int64)) > 0).all()


def test_more_tiles_than_the_scan_has_threads(cx):
    """600 000 messages: 293 source tiles and 586 destination tiles, so the byte sums, the
    zeroing and the destination scan of the one-workgroup kernels take more than one round
    per thread. Lengths only (no bytes); the expected order is numpy's stable sort."""
    import torch
    n, parts = 600_000, 5
    rng = np.random.default_rng(600)
    pl = rng.integers(0, 4, size=n).astype(np.uint32)
    ids = rng.integers(0, parts + 1, size=n).astype(np.uint32)  # (the value `parts` drops)
    src = {"payload_lengths": pl, "payload_starts": np.concatenate([[0], np.cumsum(pl, dtype=np.uint64)]).astype(np.uint64)}
    spec = _by_ids(parts, ids)
    order = np.argsort(ids, kind="stable")
    order = order[ids[order] < parts]
    first = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=parts + 1)[:parts])]).astype(np.uint64)
    starts = np.concatenate([[0], np.cumsum(pl[order], dtype=np.uint64)]).astype(np.uint64)
    keep = ("payload_lengths", "payload_starts") + EXTRA
    outs = Outs(order.size, 0, 0, parts, n, skip=[k for k in FIELDS + EXTRA if k not in keep] + ["partition_user_headers_first"])
    d_res, keepalive = _enqueue(cx, Dev(), src, n, spec, outs)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.kind == 0 and (res.count, res.dropped, res.payload_bytes) == (order.size, n - order.size, int(starts[-1]))
    got = outs.host()
    assert np.array_equal(got["source_index"], order.astype(np.uint64))
    assert np.array_equal(got["payload_lengths"], pl[order]) and np.array_equal(got["payload_starts"], starts)
    assert np.array_equal(got["partition_of"], np.where(ids < parts, ids, R.DROP).astype(np.uint32))
    assert np.array_equal(got["partition_first"], first)
    assert np.array_equal(got["partition_payload_first"], starts[first.astype(np.int64)])


# ------------------------------------------------------------------ partitions
@pytest.mark.parametrize("partitions", [1, 2, 3, 255, 256])
def test_partition_counts_by_id(cx, partitions):
    src = _source(3000, seed=partitions)
    _, got, x = _route_and_check(cx, src, R.Spec(partitions, R.KEY_ID))
    ids = src["ids"]
    for i in (0, 1, 2999):  # spelled out: xxh32(id bytes) % P
        key = int(ids[2 * i]).to_bytes(8, "little") + int(ids[2 * i + 1]).to_bytes(8, "little")
        assert int(got["partition_of"][i]) == R.xxh32(key) % partitions
    if partitions <= 3:
        assert len(set(x["partition_of"].tolist())) == partitions


def test_fewer_messages_than_partitions(cx):
    _, _, x = _route_and_check(cx, _source(100, seed=5), R.Spec(256, R.KEY_ID))
    assert (np.diff(x["partition_first"].astype(np.int64)) == 0).sum() >= 156


@pytest.mark.parametrize("partitions", [7, 256])
def test_partition_patterns(cx, partitions):
    n = TILE + 300
    i = np.arange(n)
    last = partitions - 1
    src = U.make_source(1 + i % 29, i % 4 * 3, seed=9)
    patterns = {
        "all in 0": np.zeros(n), "all in the last": np.full(n, last), "round robin": i % partitions,
        "empty at the start": 2 + i % (partitions - 2), "empty in the middle": np.where(i % 2, 0, last),
        "empty at the end": i % 3,
        # one partition's run across a wave edge (60..70) and across the tile edge (2040..2060)
        "runs": np.where(((i >= 60) & (i < 70)) | ((i >= TILE - 8) & (i < TILE + 12)), 3, i % 3),
        "drops between": np.where(i % 5 == 0, partitions, i % 2),
    }
    for name, ids in patterns.items():
        _, _, x = _route_and_check(cx, src, _by_ids(partitions, ids))
        assert x["count"] == int((ids < partitions).sum()), name
    assert x["dropped"] > 0


# ------------------------------------------------------------------ keys
@pytest.mark.parametrize("length", [1, 3, 4, 8, 15, 16, 17, 31, 32, 33, 255])
def test_bytes_keys(cx, length):
    rng = np.random.default_rng(length)
    n = 300
    src = _source(n, seed=length)
    for k, stride in enumerate((length, length + 9, length + 16)):
        keys = rng.integers(0, 256, size=(n - 1) * stride + length, dtype=np.uint8)  # ends with the last key
        spec = R.Spec(5, R.KEY_BYTES, key_length=length, key_stride=stride, keys=keys)
        shift = 1 + (length * 3 + k * 5) % 15  # the array's base misaligned by 1..15
        _, got, _ = _route_and_check(cx, src, spec, shifts={id(keys): shift})
        assert int(got["partition_of"][7]) == R.xxh32(bytes(keys[7 * stride:7 * stride + length])) % 5


def test_bytes_keys_at_every_base_misalignment(cx):
    rng = np.random.default_rng(16)
    src = _source(130, seed=16)
    for shift in range(16):
        keys = rng.integers(0, 256, size=130 * 21, dtype=np.uint8)
        _route_and_check(cx, src, R.Spec(4, R.KEY_BYTES, key_length=21, key_stride=21, keys=keys),
                         shifts={id(keys): shift})


def test_header_keys_synthetic_column(cx):
    """Keys of 1..255 B at every byte offset of the header blob, the last one ending it;
    absent to a partition and to DROP; a column entry outside its message counts as absent."""
    rng = np.random.default_rng(21)
    keys = [None if i % 6 == 0 else bytes(rng.integers(0, 256, size=[33, 1, 16, 17, 255, 4][i % 6], dtype=np.uint8))
            for i in range(400)]
    keys[-1] = bytes(rng.integers(0, 256, size=19, dtype=np.uint8))
    src, col = RU.header_source(keys)
    for shift, absent in ((0, R.DROP), (5, 0), (11, 4)):
        _, _, x = _route_and_check(cx, src, R.Spec(5, R.KEY_HEADER, absent, column=col), src_shift=shift)
        assert (x["partition_of"][:396:6] == absent).all()
    col2 = {k: v.copy() for k, v in col.items()}
    col2["value_pos"][1::7] += 300
    _, _, x = _route_and_check(cx, src, R.Spec(5, R.KEY_HEADER, 2, column=col2))
    assert int(x["partition_of"][1]) == 2


def test_header_columns_then_route(cx):
    """header_columns -> unpack_record -> route_messages on a String key of 1, 16, 17 and 255 B
    (longer than the 16-B column copy: the whole value is hashed), then on an Int32 key;
    messages without the key go to a partition or are dropped; invalid headers count as absent."""
    import user_headers_ref as H
    from iggy_amd.codec import raw_messages
    from iggy_amd.torch_io import header_columns, route_messages, unpack_record
    from oracle import oracle as O
    rng = np.random.default_rng(31)
    n = 400
    stem = bytes(rng.integers(97, 123, size=16, dtype=np.uint8))  # values sharing their first 16 B
    values = [b"k", stem, stem + b"!", stem + bytes(rng.integers(97, 123, size=239, dtype=np.uint8)), stem + b"?"]
    assert [len(v) for v in values[:4]] == [1, 16, 17, 255]
    headers, skey, ikey = [], [], []
    for i in range(n):
        parts, s, t = [], None, None
        if i % 5:
            s = values[i // 5 % len(values)]
            parts.append(H.pair(2, b"route", 2, s))
        if i % 4:
            t = int(rng.integers(-50, 150)).to_bytes(4, "little", signed=True)
            parts.append(H.pair(2, b"tenant", 6, t))
        if i % 17 == 0:  # invalid headers: every key absent
            parts, s, t = [b"\x02\x01"], None, None
        headers.append(b"".join(parts))
        skey.append(s)
        ikey.append(t)
    pls = rng.integers(0, 70, size=n).astype(np.uint32)
    uhl = np.array([len(h) for h in headers], dtype=np.uint32)
    ids = rng.integers(1, 2**63, size=2 * n, dtype=np.uint64)
    ots = (1_700_000_000_000_000 + np.arange(n)).astype(np.uint64)
    pay = rng.integers(0, 256, size=int(pls.sum()), dtype=np.uint8)
    uhb = np.frombuffer(b"".join(headers), dtype=np.uint8).copy()
    rc, e, wire = O.encode_batch(raw_messages(ids, ots, pay, pls, uhb, uhl), 3)
    assert rc == 0, e
    d_rec = to_device(np.frombuffer(wire, dtype=np.uint8).copy(), "cuda:0")
    hc = header_columns(cx, d_rec, [(2, b"route"), (2, b"tenant")])
    arrays = unpack_record(cx, d_rec)
    for col, keys, absent in ((0, skey, None), (0, skey, 1), (1, ikey, None), (1, ikey, 6)):
        want = np.array([(R.DROP if absent is None else absent) if k is None else R.xxh32(k) % 7 for k in keys],
                        dtype=np.uint32)
        order = np.concatenate([np.flatnonzero(want == p) for p in range(7)])
        r = route_messages(cx, arrays, 7, key=("header", hc["columns"][col]), absent=absent)
        assert np.array_equal(to_host(r["partition_of"]).view(np.uint32), want)
        assert np.array_equal(to_host(r["source_index"]), order) and r["count"] == order.size
        assert r["dropped"] == int((want == R.DROP).sum()) and r["examined"] == n
        assert to_host(r["user_headers"]).tobytes() == b"".join(headers[i] for i in order)
        assert np.array_equal(to_host(r["ids"]).view(np.uint64).reshape(-1), ids.reshape(-1, 2)[order].reshape(-1))
        assert r["partition_first"] == np.concatenate([[0], np.cumsum([(want == p).sum() for p in range(7)])]).tolist()
    # the 16-B, 17-B and 255-B values share their first 16 bytes: a hash of the column copy could not tell them apart
    assert len({R.xxh32(v) % 7 for v in values[1:]}) > 1


# ------------------------------------------------------------------ bytes
def test_all_payloads_empty(cx):
    src = U.make_source(np.zeros(300, np.uint32), np.arange(300) % 4, seed=3)
    _route_and_check(cx, src, R.Spec(3, R.KEY_ID))
    _route_and_check(cx, U.make_source(np.zeros(10, np.uint32), seed=4), R.Spec(2, R.KEY_ID))  # no bytes at all


def test_one_large_payload_crossing_spans(cx):
    pl = np.full(41, 5)
    pl[20] = 100_000
    src = U.make_source(pl, seed=6)
    for ids in (np.arange(41) % 3, np.where(np.arange(41) == 20, 0, 1), np.where(np.arange(41) == 20, 2, 0)):
        res, _, _ = _route_and_check(cx, src, _by_ids(3, ids))
        assert res.payload_bytes > 3 * (32 << 10)
    res, _, _ = _route_and_check(cx, src, _by_ids(3, np.where(np.arange(41) == 20, 3, 1)))  # dropped
    assert res.payload_bytes == 200


def test_more_routed_messages_under_a_span_than_its_staging_holds(cx):
    """3000 routed messages of 0..8 bytes lie under ONE 32 KiB copy span: past the 1024 starts
    a workgroup stages in LDS, so the copy searches the starts array in place."""
    rng = np.random.default_rng(9)
    src = U.make_source(rng.integers(0, 9, size=6000), rng.integers(0, 2, size=6000) * 3, seed=9)
    _, _, x = _route_and_check(cx, src, _by_ids(2, np.where(np.arange(6000) % 2, 2, np.arange(6000) // 2 % 2)))
    assert x["count"] == 3000 and x["payload_bytes"] < (32 << 10)


def test_messages_sharing_a_destination_chunk(cx):
    src = U.make_source(1 + np.arange(400) % 47, np.arange(400) % 7, seed=5)
    _route_and_check(cx, src, R.Spec(3, R.KEY_ID, mask=(np.arange(400) % 3 != 1).astype(np.uint8)))


@pytest.mark.parametrize("k", range(16))
def test_alignment(cx, k):
    """Source byte arrays at misalignment k, destination ones at (5k + 3) % 16: every source
    and every destination misalignment 0..15 (offset views of one tensor)."""
    src = U.make_source(1 + np.arange(200) % 61, np.arange(200) % 5 * 3, seed=11)
    _route_and_check(cx, src, R.Spec(3, R.KEY_ID), src_shift=k, out_shift=(5 * k + 3) % 16)


def test_without_user_headers(cx):
    src = {k: v for k, v in U.make_source(1 + np.arange(300) % 40, seed=12).items()
           if k not in ("user_headers", "user_headers_starts", "user_headers_lengths")}
    _route_and_check(cx, src, R.Spec(4, R.KEY_ID),
                     skip=("user_headers", "user_headers_starts", "user_headers_lengths", "partition_user_headers_first"))


@pytest.mark.parametrize("left_out", FIELDS[:7] + ("payloads", "user_headers") + EXTRA[1:])
def test_arrays_left_out_one_at_a_time(cx, left_out):
    _route_and_check(cx, _source(300, 12), R.Spec(3, R.KEY_ID), skip=(left_out,), exact=False)


def test_starts_left_out_with_their_bytes(cx):
    src = _source(300, 12)
    _route_and_check(cx, src, R.Spec(3, R.KEY_ID), skip=("payload_starts", "payloads", "partition_payload_first"))
    _route_and_check(cx, src, R.Spec(3, R.KEY_ID),
                     skip=("user_headers_starts", "user_headers", "partition_user_headers_first"))
    _route_and_check(cx, src, R.Spec(3, R.KEY_ID), skip=FIELDS + TABLES[1:])  # the tables and the indices alone


def test_lengths_from_the_starts(cx):
    """A source without its lengths arrays: the routed lengths are differences of the starts."""
    src = {k: v for k, v in _source(300, 13).items() if k not in ("payload_lengths", "user_headers_lengths")}
    res, _, x = _route_and_check(cx, src, R.Spec(3, R.KEY_ID), skip=("payload_lengths", "user_headers_lengths"))
    assert res.payload_bytes == x["payload_bytes"] > 0 and res.user_headers_bytes > 0


def test_source_order_against_the_copy_bound(cx):
    """The source's LAST message goes to partition 0 and its FIRST to the last partition: the
    destination order is not the source order, and the last destination bytes come from the
    source's first bytes. Short messages, so that boundary chunks are assembled from pieces."""
    for n in (2, 5, 40):
        src = U.make_source(1 + np.arange(n) % 7, 1 + np.arange(n) % 3, seed=14)
        ids = np.full(n, 1)
        ids[-1], ids[0] = 0, 2
        _, got, x = _route_and_check(cx, src, _by_ids(3, ids))
        assert x["source_index"][0] == n - 1 and x["source_index"][-1] == 0
        pl0 = int(src["payload_lengths"][0])
        assert np.array_equal(got["payloads"][x["payload_bytes"] - pl0:x["payload_bytes"]], src["payloads"][:pl0])


# ------------------------------------------------------------------ device-side errors, hash only
def test_gate_count_above_the_source_capacity(cx):
    import torch
    src = _source(100, 14)
    outs = Outs(200, 4096, 4096, 3, 200)
    d_res, keep = _enqueue(cx, Dev(), src, 101, R.Spec(3, R.KEY_ID), outs, cap=100)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (BAD, 0, 101, 0, 0)
    assert (res.examined, res.count, res.dropped, res.payload_bytes, res.user_headers_bytes, res.partitions) == \
        (101, 0, 0, 0, 0, 3)
    assert outs.untouched()


@pytest.mark.parametrize("short", ["messages", "payloads", "user_headers"])
def test_capacity(cx, short):
    import torch
    src = _source(300, 15)
    spec = R.Spec(3, R.KEY_ID, mask=(np.arange(300) % 2 == 0).astype(np.uint8))
    x = R.route(spec, src, 300)
    m, p, u = x["count"], x["payload_bytes"], x["user_headers_bytes"]
    caps = {"messages": (m - 1, p, u), "payloads": (m, p - 1, u), "user_headers": (m, p, u - 1)}[short]
    outs = Outs(*caps, 3, 300)
    d_res, keepalive = _enqueue(cx, Dev(), src, 300, spec, outs)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (abi.ERR_CAPACITY, 0, m, p, u)
    assert (res.examined, res.count, res.dropped, res.payload_bytes, res.user_headers_bytes) == (300, 0, 0, 0, 0)
    assert outs.untouched()  # no array, no table, no partition_of
    # one more of the short capacity and it fits
    outs = Outs(m, p, u, 3, 300)
    d_res, keepalive = _enqueue(cx, Dev(), src, 300, spec, outs)
    torch.cuda.synchronize()
    _check_result(_result(d_res), x, 300, 3)
    _check(outs.host(), x, 300, 3)


def test_hash_only(cx):
    """out = NULL: partition_of, partition_first (the prefix sums of the counts) and the result."""
    import torch
    src = _source(TILE + 50, 17)
    n = TILE + 50
    spec = R.Spec(5, R.KEY_ID, mask=(np.arange(n) % 7 != 0).astype(np.uint8))
    x = R.route(spec, src, n)
    outs = Outs(0, 0, 0, 5, n, skip=FIELDS + TABLES[1:] + ("source_index",))
    d_res, keepalive = _enqueue(cx, Dev(), src, n, spec, outs, hash_only=True)
    torch.cuda.synchronize()
    _check_result(_result(d_res), x, n, 5)
    got = outs.host()
    assert np.array_equal(got["partition_of"], x["partition_of"]) and np.array_equal(got["partition_first"], x["partition_first"])


def test_argument_errors_with_a_context(cx):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p, pf, pr = buf.data_ptr(), buf.data_ptr() + 1024, buf.data_ptr() + 2048  # count (0), a table, the result
    bad, good = RU.malformed_specs()
    src, ok = good["by id"]
    dev = Dev()
    s, q = dev.source(src, 3), RU.abi_spec(ok, dev.ptr)
    outs = Outs(3, 64, 64, 3, 3)
    o = outs.struct()
    call = cx.route_messages_device
    assert call(s, p, q, o, pf, None, None, None, None, pr) == 0
    torch.cuda.synchronize()
    assert call(s, None, q, o, pf, None, None, None, None, pr) == BAD          # d_count
    assert call(s, p, q, o, None, None, None, None, None, pr) == BAD         # d_partition_first
    assert call(s, p, q, o, pf, None, None, None, None, None) == BAD         # the result
    L = cx._L
    assert L.iggy_codec_route_messages_device(cx._h, None, p, ctypes.byref(q), None, pf, None, None, None, None, pr, None) == BAD
    assert L.iggy_codec_route_messages_device(cx._h, ctypes.byref(s), p, None, None, pf, None, None, None, None, pr, None) == BAD
    for name, (hsrc, spec) in bad.items():
        d = Dev()
        assert call(d.source(hsrc, 3), p, RU.abi_spec(spec, d.ptr), None, pf, None, None, None, None, pr) == BAD, name
    for name, (hsrc, spec) in good.items():
        d = Dev()
        assert call(d.source(hsrc, 3), p, RU.abi_spec(spec, d.ptr), None, pf, None, None, None, None, pr) == 0, name
    torch.cuda.synchronize()
    # the select's refusals for out: an array wanted and missing in src, or equal to it; bytes without their starts
    for k in FIELDS:
        d = Dev()
        assert call(d.source({x: v for x, v in src.items() if x != k}, 3), p, q, o, pf, None, None, None, None, pr) == BAD, k
        same = outs.struct()
        setattr(same, k, getattr(s, k))
        assert call(s, p, q, same, pf, None, None, None, None, pr) == BAD, k
    for b, st, tab in (("payloads", "payload_starts", 5), ("user_headers", "user_headers_starts", 6)):
        o2 = outs.struct()
        setattr(o2, st, None)
        assert call(s, p, q, o2, pf, None, None, None, None, pr) == BAD, b
        setattr(o2, b, None)
        assert call(s, p, q, o2, pf, None, None, None, None, pr) == 0, b
        args = [s, p, q, o2, pf, None, None, None, None, pr]
        args[tab] = pf  # a byte table without its starts array in out
        assert call(*args) == BAD, b
    # a byte table or the source index without out
    assert call(s, p, q, None, pf, pf, None, None, None, pr) == BAD
    assert call(s, p, q, None, pf, None, pf, None, None, pr) == BAD
    assert call(s, p, q, None, pf, None, None, None, pf, pr) == BAD
    torch.cuda.synchronize()
    outs.host()  # guards


# ------------------------------------------------------------------ determinism
def test_determinism(cx):
    src = U.make_source(np.random.default_rng(51).integers(0, 300, size=5000), np.arange(5000) % 4 * 9, seed=51)
    spec = R.Spec(16, R.KEY_ID, mask=(np.random.default_rng(52).random(5000) < 0.8).astype(np.uint8))
    x = R.route(spec, src, 5000)
    _, a, _ = _route_and_check(cx, src, spec, x=x)
    _, b, _ = _route_and_check(cx, src, spec, x=x)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------ re-batch round trip, chain
def test_rebatch_round_trip(cx):
    """unpack_record -> route_messages by id into 3 partitions -> encode_device of each raw(p)
    with partition_id = p: byte-equal to the oracle's encode_batch of the same messages built
    on the host, and accepted by a Verify decode."""
    import torch
    from iggy_amd.codec import raw_messages
    from iggy_amd.torch_io import route_messages, unpack_record
    from oracle import oracle as O
    rec = O.synth_batch(600, 0, 700, 9, seed=62)
    rc, e, msgs = O.poll_decode(rec, 1)
    assert rc == 0 and len(msgs) == 600, e
    part = [R.xxh32(m.id_lo.to_bytes(8, "little") + m.id_hi.to_bytes(8, "little")) % 3 for m in msgs]
    assert all(part.count(p) > 0 for p in range(3))  # by the restatement alone
    arrays = unpack_record(cx, to_device(rec, "cuda:0"))
    r = route_messages(cx, arrays, 3)
    assert (r["count"], r["dropped"], r["examined"]) == (600, 0, 600)
    assert to_host(r["partition_of"]).tolist() == part
    assert r["partition_first"] == [0, part.count(0), part.count(0) + part.count(1), 600]
    s = torch.cuda.current_stream().cuda_stream
    for p in range(3):
        mine = [m for m, q in zip(msgs, part) if q == p]
        ids = np.array([[m.id_lo, m.id_hi] for m in mine], dtype=np.uint64).reshape(-1)
        ots = np.array([m.origin_timestamp for m in mine], dtype=np.uint64)
        pls = np.array([m.payload_length for m in mine], dtype=np.uint32)
        uhl = np.array([m.user_headers_length for m in mine], dtype=np.uint32)
        pay = np.concatenate([rec[m.payload_pos:m.payload_pos + m.payload_length] for m in mine])
        uhb = np.concatenate([rec[m.user_headers_pos:m.user_headers_pos + m.user_headers_length] for m in mine])
        rc, e, wire = O.encode_batch(raw_messages(ids, ots, pay, pls, uhb, uhl), p)
        assert rc == 0, e
        d_out = torch.full((len(wire) + 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
        d_er = torch.zeros(ctypes.sizeof(abi.EncodeResult), dtype=torch.uint8, device="cuda:0")
        assert cx.encode_device(r["raw"](p), p, d_out.data_ptr(), len(wire), d_er.data_ptr(), s) == 0
        torch.cuda.synchronize()
        er = abi.EncodeResult.from_buffer_copy(to_host(d_er).tobytes())
        assert er.error.kind == 0 and er.batch_length == len(wire)
        out = to_host(d_out)
        assert out[:len(wire)].tobytes() == wire and (out[len(wire):] == 0xCD).all()
        rc, e, h, frames = cx.decode_batch_slice_with(out[:len(wire)].copy(), abi.INTEGRITY_VERIFY)
        assert rc == 0 and h.message_count == len(mine) and h.partition_id == p, e


def test_select_then_route_chain(cx):
    """select -> route queued back to back: the route reads its count at &select_result->count."""
    import torch
    n = 700
    src = _source(n, 81)
    keep = (np.arange(n) % 3 != 0).astype(np.uint8)
    kept = SR.select(src, n, [], keep)
    mid = {k: kept[k] for k in FIELDS}
    spec = R.Spec(4, R.KEY_ID)
    x = R.route(spec, mid, kept["count"])
    dev = Dev()
    sel_out = {k: torch.zeros(max(np.asarray(src[k]).nbytes + (8 if k.endswith("_starts") else 0), 8),
                              dtype=torch.uint8, device="cuda:0") for k in FIELDS}
    so = abi.UnpackedMessages(n, src["payloads"].size, src["user_headers"].size, *(sel_out[k].data_ptr() for k in FIELDS))
    d_cnt = to_device(np.array([n], dtype=np.int64), "cuda:0")
    d_sel = torch.zeros(ctypes.sizeof(abi.SelectResult), dtype=torch.uint8, device="cuda:0")
    d_res = torch.full((ctypes.sizeof(abi.RouteResult),), 0xEE, dtype=torch.uint8, device="cuda:0")
    outs = Outs(x["count"], x["payload_bytes"], x["user_headers_bytes"], 4, n)
    s = torch.cuda.current_stream().cuda_stream
    assert cx.select_messages_device(dev.source(src, n), d_cnt.data_ptr(), U.abi_spec([], dev.ptr, keep), so, None,
                                     None, d_sel.data_ptr(), s) == 0
    q = RU.abi_spec(spec, dev.ptr)
    assert cx.route_messages_device(so, d_sel.data_ptr() + abi.SelectResult.count.offset, q, outs.struct(),
                                    outs.ptr("partition_first"), outs.ptr("partition_payload_first"),
                                    outs.ptr("partition_user_headers_first"), outs.ptr("partition_of"),
                                    outs.ptr("source_index"), d_res.data_ptr(), s) == 0
    torch.cuda.synchronize()  # the only one
    _check_result(_result(d_res), x, kept["count"], 4)
    _check(outs.host(), x, kept["count"], 4)
