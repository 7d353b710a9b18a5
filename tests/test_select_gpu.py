"""GPU tests of the device select (iggy_codec_select_messages_device, select.hip): typed
clauses over unpacked arrays and header columns, then the stable compaction of the kept
messages into a second set of arrays.

Expected values come from the plain numpy restatement (tests/select_ref.py) alone. Inputs
are numpy arrays put on the device with torch_io.to_device; the header columns are
synthetic numpy columns, so this file, apart from its last test, does not run the
user-header kernels. Every output array, the source index included, sits between 0xA5
guards that must survive every call, errors included. Integer byte work: every comparison
is bit-exact."""
import ctypes

import numpy as np
import pytest

import select_ref as R
import select_util as U
from iggy_amd import abi
from iggy_amd.torch_io import to_device, to_host

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
U64 = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_starts", "user_headers_starts",
       "source_index")
U32 = ("payload_lengths", "user_headers_lengths")
BYTES = ("payloads", "user_headers")
FIELDS = U.FIELDS
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
    shift: the payloads / user_headers arrays start `shift` bytes into their tensors."""

    def __init__(self, shift=0):
        self.t, self.shift = {}, shift

    def ptr(self, a, byte_array=False):
        key = id(a)
        if key not in self.t:
            flat = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            sh = self.shift if byte_array else 0
            buf = np.zeros(max(flat.size + sh, 1), np.uint8)
            buf[sh:sh + flat.size] = flat
            self.t[key] = (to_device(buf, "cuda:0"), sh, a)
        t, sh, _ = self.t[key]
        return t.data_ptr() + sh

    def source(self, src, cap, cap_p=None, cap_u=None):
        bytes_ids = {id(src[k]) for k in BYTES if src.get(k) is not None}
        return U.src_struct(src, cap, lambda a: self.ptr(a, id(a) in bytes_ids), cap_p, cap_u)


class Outs:
    """Every output array, and the source index, as [front guard | capacity | back guard] of 0xA5."""

    def __init__(self, cap_m, cap_p, cap_u, shift=0, skip=()):
        import torch
        self.cap = (cap_m, cap_p, cap_u)
        self.t, self.front, self.size = {}, {}, {}
        for k in FIELDS + ("source_index",):
            if k in skip:
                continue
            if k in BYTES:
                size, front = (cap_p if k == "payloads" else cap_u), GUARD + shift
            elif k in U32:
                size, front = 4 * cap_m, GUARD
            elif k == "ids":
                size, front = 16 * cap_m, GUARD
            elif k.endswith("_starts"):
                size, front = 8 * (cap_m + 1), GUARD
            else:
                size, front = 8 * cap_m, GUARD
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

    def untouched(self):
        return all((to_host(t) == FILL).all() for t in self.t.values())


def _cursor(m=0, p=0, u=0):
    return to_device(np.array([m, p, u, 0], dtype=np.int64), "cuda:0")


def _enqueue(cx, dev, src, count, clauses, outs, mask=None, cursor=None, cap=None, cap_p=None, cap_u=None):
    """One select on the current stream, no synchronise -> (result tensor, keep-alive)."""
    import torch
    s = dev.source(src, count if cap is None else cap, cap_p, cap_u)
    spec = U.abi_spec(clauses, dev.ptr, mask)
    d_cnt = to_device(np.array([count], dtype=np.int64), "cuda:0")
    d_res = torch.full((ctypes.sizeof(abi.SelectResult),), 0xEE, dtype=torch.uint8, device="cuda:0")
    rc = cx.select_messages_device(s, d_cnt.data_ptr(), spec, outs.struct(), outs.ptr("source_index"),
                                   cursor.data_ptr() if cursor is not None else None, d_res.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return d_res, (d_cnt, s, spec)


def _result(d_res):
    return abi.SelectResult.from_buffer_copy(to_host(d_res).tobytes())


def _check(got, x, first=0, base_p=0, base_u=0):
    n = x["count"]
    for k in ("checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths", "user_headers_lengths",
              "source_index"):
        if k in got and k in x:
            assert np.array_equal(got[k][first:first + n], x[k]), k
    if "ids" in got:
        assert np.array_equal(got["ids"][2 * first:2 * (first + n)], x["ids"])
    for k in ("payload_starts", "user_headers_starts"):
        if k in got:
            assert np.array_equal(got[k][first:first + n + 1], x[k]), k
    if "payloads" in got:
        assert np.array_equal(got["payloads"][base_p:base_p + x["payloads"].size], x["payloads"])
    if "user_headers" in got:
        assert np.array_equal(got["user_headers"][base_u:base_u + x["user_headers"].size], x["user_headers"])


def _check_result(res, x, examined):
    assert res.error.astuple() == (0, 0, 0, 0, 0), res.error
    assert (res.examined, res.count, res.payload_bytes, res.user_headers_bytes, res.first_message) == \
        (examined, x["count"], x["payload_bytes"], x["user_headers_bytes"], x["first_message"])
    assert (res.min_payload_length, res.max_payload_length) == (x["min_payload_length"], x["max_payload_length"])


def _select_and_check(cx, src, keep, clauses=(), src_shift=0, out_shift=0, slack=0, skip=(), exact=False):
    """The select of `src` with the keep pattern as its mask (and clauses), against the restatement."""
    import torch
    n = src["payload_lengths"].size if src.get("payload_lengths") is not None else src["payload_starts"].size - 1
    mask = None if keep is None else np.asarray(keep, dtype=np.uint8)
    x = R.select(src, n, list(clauses), mask)
    if exact:  # capacities of exactly what is kept
        outs = Outs(x["count"], x["payload_bytes"], x["user_headers_bytes"], out_shift, skip)
    else:
        outs = Outs(n + slack, src["payloads"].size + slack, src["user_headers"].size + slack, out_shift, skip)
    dev = Dev(src_shift)
    d_res, keepalive = _enqueue(cx, dev, src, n, list(clauses), outs, mask)
    torch.cuda.synchronize()
    res = _result(d_res)
    _check_result(res, x, n)
    got = outs.host()
    _check(got, x)
    return res, got, x


def _source(n, seed=1):
    return U.make_source(np.arange(n) % 23, np.where(np.arange(n) % 3 == 0, 5, 0), seed)


# ------------------------------------------------------------------ counts and keep patterns
def _patterns(n):
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": i % 2 == 1, "first": i == 0,
            "last": i == n - 1}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, 3 * 256 + 1])
def test_counts_and_keep_patterns(cx, n):
    src = _source(n, seed=n + 1)
    for name, keep in _patterns(n).items():
        res, _, x = _select_and_check(cx, src, keep, slack=2)
        assert x["count"] == int(keep.sum()), name
    _select_and_check(cx, src, None)  # no mask, no clause: everything is kept


def test_kept_run_straddling_a_tile_edge(cx):
    i = np.arange(3 * 256 + 1)
    _select_and_check(cx, _source(i.size, 7), (i >= 250) & (i < 262))
    _select_and_check(cx, _source(i.size, 7), (i >= 500) & (i < 769))


def test_empty_tile_between_two_kept_tiles(cx):
    i = np.arange(3 * 256 + 1)
    _, _, x = _select_and_check(cx, _source(i.size, 8), (i < 256) | (i >= 512))
    assert x["count"] == 256 + 257


# ------------------------------------------------------------------ bytes
def test_all_payloads_empty(cx):
    src = U.make_source(np.zeros(300, np.uint32), np.arange(300) % 4, seed=3)
    _select_and_check(cx, src, np.arange(300) % 2 == 0)
    _select_and_check(cx, U.make_source(np.zeros(10, np.uint32), seed=4), np.ones(10, bool))


def test_messages_sharing_a_destination_chunk(cx):
    src = U.make_source(1 + np.arange(400) % 47, np.arange(400) % 7, seed=5)
    _select_and_check(cx, src, np.arange(400) % 3 != 1, exact=True)


def test_one_large_payload_crossing_spans(cx):
    pl = np.full(41, 5)
    pl[20] = 100_000
    src = U.make_source(pl, seed=6)
    keep = np.ones(41, bool)
    res, _, _ = _select_and_check(cx, src, keep, exact=True)          # kept: crosses 32 KiB spans
    assert res.max_payload_length == 100_000 and res.payload_bytes > 3 * (32 << 10)
    keep[20] = False
    res, _, _ = _select_and_check(cx, src, keep, exact=True)          # dropped: 200 bytes around it
    assert res.payload_bytes == 200
    keep[:] = False
    keep[20] = True
    _select_and_check(cx, src, keep, exact=True)                      # alone


def test_more_kept_messages_under_a_span_than_its_staging_holds(cx):
    """3000 kept messages of 0..8 bytes lie under ONE 32 KiB copy span: past the 1024 starts
    a workgroup stages in LDS, so the copy searches the starts array in place."""
    rng = np.random.default_rng(9)
    src = U.make_source(rng.integers(0, 9, size=6000), rng.integers(0, 2, size=6000) * 3, seed=9)
    _, _, x = _select_and_check(cx, src, np.arange(6000) % 2 == 0, exact=True)
    assert x["count"] == 3000 and x["payload_bytes"] < (32 << 10)


def test_kept_message_is_the_sources_last(cx):
    """The only kept bytes end the source arrays: wide loads must stay inside them."""
    src = U.make_source([40, 3, 9, 1, 5], [0, 0, 7, 0, 3], seed=10)
    for last in (np.array([0, 0, 0, 0, 1], bool), np.array([0, 0, 1, 1, 1], bool), np.array([0, 1, 0, 0, 1], bool)):
        _select_and_check(cx, src, last, exact=True)


@pytest.mark.parametrize("k", range(16))
def test_alignment(cx, k):
    """Source byte arrays at misalignment k, destination ones at (5k + 3) % 16: every
    source and every destination misalignment 0..15 (offset views of one tensor)."""
    src = U.make_source(1 + np.arange(200) % 61, np.arange(200) % 5 * 3, seed=11)
    _select_and_check(cx, src, np.arange(200) % 3 != 0, src_shift=k, out_shift=(5 * k + 3) % 16, exact=True)


# ------------------------------------------------------------------ array choice
@pytest.mark.parametrize("left_out", FIELDS[:7] + ("payloads", "user_headers", "source_index"))
def test_arrays_left_out_one_at_a_time(cx, left_out):
    _select_and_check(cx, _source(300, 12), np.arange(300) % 2 == 0, skip=(left_out,))


def test_starts_left_out_with_their_bytes(cx):
    _select_and_check(cx, _source(300, 12), np.arange(300) % 2 == 0, skip=("payload_starts", "payloads"))
    _select_and_check(cx, _source(300, 12), np.arange(300) % 2 == 0, skip=("user_headers_starts", "user_headers"))
    _select_and_check(cx, _source(300, 12), np.arange(300) % 2 == 0, skip=FIELDS)  # the source index alone


def test_lengths_from_the_starts(cx):
    """A source without its lengths arrays: the kept lengths are differences of the starts."""
    src = {k: v for k, v in _source(300, 13).items() if k not in ("payload_lengths", "user_headers_lengths")}
    res, got, x = _select_and_check(cx, src, np.arange(300) % 3 == 0, skip=("payload_lengths", "user_headers_lengths"))
    assert res.payload_bytes == x["payload_bytes"] > 0 and res.user_headers_bytes > 0


# ------------------------------------------------------------------ device-side errors
def test_gate_count_above_the_source_capacity(cx):
    import torch
    src = _source(100, 14)
    outs = Outs(200, 4096, 4096)
    cur = _cursor(2, 7, 3)
    d_res, keep = _enqueue(cx, Dev(), src, 101, [], outs, None, cur, cap=100)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (BAD, 0, 101, 0, 0)
    assert (res.examined, res.count, res.payload_bytes, res.user_headers_bytes, res.first_message) == (101, 0, 0, 0, 2)
    assert outs.untouched()
    assert to_host(cur).tolist() == [2, 7, 3, 0]


@pytest.mark.parametrize("short", ["messages", "payloads", "user_headers"])
def test_capacity(cx, short):
    import torch
    src = _source(300, 15)
    keep = (np.arange(300) % 2 == 0).astype(np.uint8)
    x = R.select(src, 300, [], keep)
    m, p, u = 5 + x["count"], 11 + x["payload_bytes"], 4 + x["user_headers_bytes"]  # bases included
    caps = {"messages": (m - 1, p, u), "payloads": (m, p - 1, u), "user_headers": (m, p, u - 1)}[short]
    outs = Outs(*caps)
    cur = _cursor(5, 11, 4)
    d_res, keepalive = _enqueue(cx, Dev(), src, 300, [], outs, keep, cur)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (abi.ERR_CAPACITY, 0, m, p, u)
    assert (res.examined, res.count, res.payload_bytes, res.user_headers_bytes, res.first_message) == (300, 0, 0, 0, 5)
    assert outs.untouched()
    assert to_host(cur).tolist() == [5, 11, 4, 0]
    # one more of the short capacity and it fits
    outs = Outs(m, p, u)
    d_res, keepalive = _enqueue(cx, Dev(), src, 300, [], outs, keep, cur)
    torch.cuda.synchronize()
    assert _result(d_res).error.kind == 0 and to_host(cur).tolist() == [m, p, u, 0]
    _check(outs.host(), R.select(src, 300, [], keep, 5, 11, 4), 5, 11, 4)


def test_argument_errors_with_a_context(cx):
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    src = _source(3, 16)
    dev = Dev()
    s = dev.source(src, 3)
    ok_spec = U.abi_spec([], dev.ptr)
    outs = Outs(3, 64, 64)
    o = outs.struct()
    call = cx.select_messages_device
    assert call(s, p, ok_spec, o, None, None, p) == 0
    torch.cuda.synchronize()
    assert call(s, None, ok_spec, o, None, None, p) == BAD
    assert call(s, p, ok_spec, o, None, None, None) == BAD
    L = cx._L
    assert L.iggy_codec_select_messages_device(cx._h, None, p, ctypes.byref(ok_spec), ctypes.byref(o), None, None, p, None) == BAD
    assert L.iggy_codec_select_messages_device(cx._h, ctypes.byref(s), p, None, ctypes.byref(o), None, None, p, None) == BAD
    assert L.iggy_codec_select_messages_device(cx._h, ctypes.byref(s), p, ctypes.byref(ok_spec), None, None, None, p, None) == BAD
    bad, good = U.malformed_specs()
    for name, (hsrc, clauses) in bad.items():
        d = Dev()
        assert call(d.source(hsrc, 3), p, U.abi_spec(clauses, d.ptr), abi.UnpackedMessages(3, 0, 0), None, None, p) == BAD, name
    # an array wanted in out and missing in src, or equal to it; bytes without their starts
    for k in FIELDS:
        d = Dev()
        assert call(d.source({x: v for x, v in src.items() if x != k}, 3), p, ok_spec, o, None, None, p) == BAD, k
        same = outs.struct()
        setattr(same, k, getattr(s, k))
        assert call(s, p, ok_spec, same, None, None, p) == BAD, k
    for b, st in (("payloads", "payload_starts"), ("user_headers", "user_headers_starts")):
        o2 = outs.struct()
        setattr(o2, st, None)
        assert call(s, p, ok_spec, o2, None, None, p) == BAD, b
    torch.cuda.synchronize()
    outs.host()  # guards


# ------------------------------------------------------------------ chaining
def test_cursor_chain_of_three_selects(cx):
    import torch
    parts = [(_source(300, 21), np.arange(300) % 2 == 0), (U.make_source(1 + np.arange(70) % 47, seed=22), np.ones(70, bool)),
             (_source(513, 23), np.arange(513) % 5 == 1)]
    xs, first, bp, bu = [], 0, 0, 0
    for src, keep in parts:
        x = R.select(src, keep.size, [], keep.astype(np.uint8), first, bp, bu)
        xs.append(x)
        first, bp, bu = first + x["count"], bp + x["payload_bytes"], bu + x["user_headers_bytes"]
    outs = Outs(first, bp, bu)
    cur = _cursor()
    queued = [_enqueue(cx, Dev(), src, keep.size, [], outs, keep.astype(np.uint8), cur) for src, keep in parts]
    torch.cuda.synchronize()  # the only one
    got = outs.host()
    for (d_res, keepalive), x, (src, keep) in zip(queued, xs, parts):
        _check_result(_result(d_res), x, keep.size)
        _check(got, x, x["first_message"], int(x["payload_starts"][0]), int(x["user_headers_starts"][0]))
    assert to_host(cur).tolist() == [first, bp, bu, 0]
    assert got["payload_starts"][first] == bp and got["user_headers_starts"][first] == bu


def test_select_appended_after_an_unpack(cx):
    import torch
    from oracle import oracle as O
    rec = O.synth_batch(300, 10, 90, 3, seed=31)
    rc, e, msgs = O.poll_decode(rec, 1)
    assert rc == 0, e
    up_p = sum(m.payload_length for m in msgs)
    up_u = sum(m.user_headers_length for m in msgs)
    src, keep = _source(257, 32), (np.arange(257) % 2 == 1).astype(np.uint8)
    x = R.select(src, 257, [], keep, 300, up_p, up_u)
    outs = Outs(300 + x["count"], up_p + x["payload_bytes"], up_u + x["user_headers_bytes"])
    cur = _cursor()
    d_rec = to_device(rec, "cuda:0")
    n = rec.size
    d_pos = torch.zeros(n // 48 + 1, dtype=torch.int64, device="cuda:0")
    d_dec = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device="cuda:0")
    d_ur = torch.zeros(ctypes.sizeof(abi.UnpackResult), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    assert cx.decode_device(d_rec.data_ptr(), n, 0, d_pos.data_ptr(), n // 48 + 1, d_dec.data_ptr(), s) == 0
    assert cx.unpack_device(d_rec.data_ptr(), n, d_pos.data_ptr(), d_dec.data_ptr(), outs.struct(), cur.data_ptr(),
                            d_ur.data_ptr(), s) == 0
    d_res, keepalive = _enqueue(cx, Dev(), src, 257, [], outs, keep, cur)
    torch.cuda.synchronize()
    ur = abi.UnpackResult.from_buffer_copy(to_host(d_ur).tobytes())
    assert ur.error.kind == 0 and (ur.count, ur.payload_bytes, ur.user_headers_bytes) == (300, up_p, up_u)
    _check_result(_result(d_res), x, 257)
    got = outs.host()
    _check(got, x, 300, up_p, up_u)
    assert [m.offset for m in msgs] == got["offsets"][:300].tolist()  # the unpack's part stays
    assert np.array_equal(got["payloads"][:up_p], np.concatenate([rec[m.payload_pos:m.payload_pos + m.payload_length] for m in msgs]))
    assert to_host(cur).tolist() == [300 + x["count"], up_p + x["payload_bytes"], up_u + x["user_headers_bytes"], 0]


# ------------------------------------------------------------------ clauses
def _verdicts(cx, dev, src, n, clauses, mask=None):
    """The kept source indices of one select that wants the source index alone."""
    import torch
    outs = Outs(n, 0, 0, skip=FIELDS)
    d_res, keepalive = _enqueue(cx, dev, src, n, clauses, outs, mask)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.kind == 0 and res.examined == n
    return outs.host()["source_index"][:res.count]


def test_plain_sources_at_their_boundaries(cx):
    src, clauses = U.plain_cases()
    n = src["offsets"].size
    dev = Dev()
    for c in clauses:
        want = np.flatnonzero(R.keep_mask(src, n, [c])).astype(np.uint64)
        assert np.array_equal(_verdicts(cx, dev, src, n, [c]), want), c


@pytest.mark.parametrize("group", ["signed", "unsigned", "float32", "float64", "bool", "text"])
def test_header_kinds_at_their_boundaries(cx, group):
    """The CPU boundary table through the device: one test per kind group, one small select
    per op and operand (all of a group's columns are uploaded once)."""
    dev = Dev()
    for g, col, clauses in U.header_cases():
        if g != group:
            continue
        n = col["value_kinds"].size
        for c in clauses:
            want = np.flatnonzero(R.keep_mask({}, n, [c])).astype(np.uint64)
            assert np.array_equal(_verdicts(cx, dev, {}, n, [c]), want), (c.kind, c.op, c.operand.hex())


def test_mask_anded_with_two_clauses(cx):
    src = _source(600, 41)
    tenant = U.column([(R.K_INT32, 4, U._i(int(v), 4, True)) if v % 7 else (0, 0, b"") for v in range(-300, 300)])
    clauses = [R.clause(R.SEL_HEADER, R.OP_GE, U._i(-100, 4, True), R.K_INT32, tenant),
               R.clause(R.SEL_PAYLOAD_LENGTH, R.OP_LT, U._i(15, 4, False))]
    keep = np.arange(600) % 3 != 0
    _, _, x = _select_and_check(cx, src, keep, clauses)
    assert 0 < x["count"] < int(keep.sum())
    status = np.zeros((600, 4), np.uint32)
    status[::11, 0] = 2
    _, _, y = _select_and_check(cx, src, keep, clauses + [R.clause(R.SEL_HEADER_STATUS, status=status)])
    assert 0 < y["count"] < x["count"]


def test_seeded_mix(cx):
    src, specs = U.seeded_mix()
    n = src["offsets"].size
    dev = Dev()
    for clauses, mask in specs:
        want = np.flatnonzero(R.keep_mask(src, n, clauses, mask)).astype(np.uint64)
        assert np.array_equal(_verdicts(cx, dev, src, n, clauses, mask), want)


def test_determinism(cx):
    src = U.make_source(np.random.default_rng(51).integers(0, 300, size=2000), np.arange(2000) % 4 * 9, seed=51)
    keep = np.random.default_rng(52).random(2000) < 0.5
    _, a, _ = _select_and_check(cx, src, keep)
    _, b, _ = _select_and_check(cx, src, keep)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------ re-batch round trip
@pytest.mark.parametrize("shape", ["uniform", "mixed"])
def test_rebatch_round_trip(cx, shape):
    """unpack_record -> select (offset parity as a mask, a payload-length range as clauses) ->
    encode_device -> a Verify decode; the encoded bytes equal the oracle's encode_batch of the
    same kept messages built on the host."""
    import torch
    from iggy_amd.codec import raw_messages
    from iggy_amd.torch_io import select_clause, select_messages, unpack_record
    from oracle import oracle as O
    rec = O.synth_batch(600, 256, 256, seed=61) if shape == "uniform" else O.synth_batch(500, 0, 700, 9, seed=62)
    rc, e, msgs = O.poll_decode(rec, 1)
    assert rc == 0, e
    lo, hi = (256, 256) if shape == "uniform" else (100, 500)
    kept = [m for m in msgs if m.offset % 2 == 1 and lo <= m.payload_length <= hi]
    assert 0 < len(kept) < len(msgs)
    arrays = unpack_record(cx, to_device(rec, "cuda:0"))
    mask = (arrays["offsets"] & 1).to(torch.uint8)
    sel = select_messages(cx, arrays, [select_clause("payload_length", ">=", lo),
                                       select_clause("payload_length", "<=", hi)], mask=mask)
    assert sel["count"] == len(kept) and sel["examined"] == len(msgs)
    assert to_host(sel["offsets"]).astype(np.uint64).tolist() == [m.offset for m in kept]
    assert to_host(sel["source_index"]).tolist() == [i for i, m in enumerate(msgs) if m in kept]
    # the oracle's encode of the same messages, built on the host
    ids = np.array([[m.id_lo, m.id_hi] for m in kept], dtype=np.uint64).reshape(-1)
    ots = np.array([m.origin_timestamp for m in kept], dtype=np.uint64)
    pls = np.array([m.payload_length for m in kept], dtype=np.uint32)
    uhl = np.array([m.user_headers_length for m in kept], dtype=np.uint32)
    pay = np.concatenate([rec[m.payload_pos:m.payload_pos + m.payload_length] for m in kept])
    uhb = np.concatenate([rec[m.user_headers_pos:m.user_headers_pos + m.user_headers_length] for m in kept])
    raw = raw_messages(ids, ots, pay, pls, uhb if uhb.size else None, uhl if uhb.size else None)
    rc, e, wire = O.encode_batch(raw, 0)
    assert rc == 0, e
    d_out = torch.full((len(wire) + 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
    d_er = torch.zeros(ctypes.sizeof(abi.EncodeResult), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    assert cx.encode_device(sel["raw"], 0, d_out.data_ptr(), len(wire), d_er.data_ptr(), s) == 0
    torch.cuda.synchronize()
    er = abi.EncodeResult.from_buffer_copy(to_host(d_er).tobytes())
    assert er.error.kind == 0 and er.batch_length == len(wire)
    out = to_host(d_out)
    assert out[:len(wire)].tobytes() == wire and (out[len(wire):] == 0xCD).all()
    rc, e, h, frames = cx.decode_batch_slice_with(out[:len(wire)].copy(), abi.INTEGRITY_VERIFY)
    assert rc == 0 and h.message_count == len(kept), e


# ------------------------------------------------------------------ header chain
def test_header_columns_then_select(cx):
    """decode -> header columns -> unpack -> select on a String key and an Int32 range,
    against user_headers_ref plus select_ref. Apart from the rest of this file because it is
    the one test here that runs the user-header kernels."""
    import user_headers_ref as H
    from iggy_amd.codec import raw_messages
    from iggy_amd.torch_io import header_columns, select_clause, select_messages, unpack_record
    from oracle import oracle as O
    rng = np.random.default_rng(71)
    n = 400
    headers = []
    for i in range(n):
        parts = []
        if i % 5:
            parts.append(H.pair(2, b"route", 2, [b"eu", b"us", b"eu-central-1-long-zone"][i % 3]))
        if i % 4:
            parts.append(H.pair(2, b"tenant", 6, int(rng.integers(-50, 150)).to_bytes(4, "little", signed=True)))
        headers.append(b"".join(parts) if i % 17 else b"\x02\x01")  # every 17th: invalid headers
    pls = rng.integers(0, 70, size=n).astype(np.uint32)
    uhl = np.array([len(h) for h in headers], dtype=np.uint32)
    ids = rng.integers(1, 2**63, size=2 * n, dtype=np.uint64)  # (raw_messages holds addresses: the arrays stay named)
    ots = (1_700_000_000_000_000 + np.arange(n)).astype(np.uint64)
    pay = rng.integers(0, 256, size=int(pls.sum()), dtype=np.uint8)
    uhb = np.frombuffer(b"".join(headers), dtype=np.uint8).copy()
    raw = raw_messages(ids, ots, pay, pls, uhb, uhl)
    rc, e, wire = O.encode_batch(raw, 3)
    assert rc == 0, e
    rec = np.frombuffer(wire, dtype=np.uint8).copy()
    keys = [(2, b"route"), (2, b"tenant")]
    # the restatement: columns from user_headers_ref, the verdicts from select_ref
    decoded = [H.decode(h) for h in headers]
    cols = [U.column([(lambda v: (v[0], v[2], v[3]))(H.lookup(d, k)) for d in decoded]) for k in keys]
    status = np.array([d[0] for d in decoded], dtype=np.uint32)
    clauses = [R.clause(R.SEL_HEADER, R.OP_EQ, b"eu", R.K_STRING, cols[0]),
               R.clause(R.SEL_HEADER, R.OP_GE, U._i(0, 4, True), R.K_INT32, cols[1]),
               R.clause(R.SEL_HEADER, R.OP_LT, U._i(100, 4, True), R.K_INT32, cols[1]),
               R.clause(R.SEL_HEADER_STATUS, status=status)]
    want = np.flatnonzero(R.keep_mask({}, n, clauses))
    assert 10 < want.size < n // 2
    d_rec = to_device(rec, "cuda:0")
    hc = header_columns(cx, d_rec, keys)
    arrays = unpack_record(cx, d_rec)
    sel = select_messages(cx, arrays, [
        select_clause(hc["columns"][0], "==", b"eu", abi.KIND_STRING),
        select_clause(hc["columns"][1], ">=", 0, abi.KIND_INT32),
        select_clause(hc["columns"][1], "<", 100, abi.KIND_INT32),
        select_clause(hc["status"])])
    assert to_host(sel["source_index"]).tolist() == want.tolist()
    assert sel["count"] == want.size
    assert to_host(sel["user_headers"]).tobytes() == b"".join(headers[i] for i in want)
