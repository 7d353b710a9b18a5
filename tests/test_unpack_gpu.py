"""GPU tests of the consumer unpack (iggy_codec_unpack_batch_device, unpack.hip): a
decoded device-resident record back into struct-of-arrays tensors.

The expected arrays come from the oracle alone: O.poll_decode(rec, mode=1) gives the
resolved descriptors, the expected payloads / user headers are the record's own bytes at
the descriptors' positions, the starts their numpy cumulative sums. Every output array
sits between 0xA5 guards that must survive every case, errors included. Integer byte
work: every comparison is bit-exact."""
import ctypes

import numpy as np
import pytest

from iggy_amd import abi
from iggy_amd.torch_io import to_device, to_host
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
U64 = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_starts", "user_headers_starts")
U32 = ("payload_lengths", "user_headers_lengths")
BYTES = ("payloads", "user_headers")
FIELDS = ("ids", "checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths",
          "user_headers_lengths", "payload_starts", "user_headers_starts", "payloads", "user_headers")


@pytest.fixture(scope="module")
def cx():
    from iggy_amd.codec import Codec
    c = Codec(0)
    yield c
    c.close()


# ------------------------------------------------------------------ records
def _mkraw(pls, uhl=None, seed=1):
    from iggy_amd.codec import raw_messages
    rng = np.random.default_rng(seed)
    pls = np.asarray(pls, dtype=np.uint32)
    n = pls.size
    ids = rng.integers(1, 2**63, size=2 * n, dtype=np.uint64)
    ots = (1_700_000_000_000_000 + rng.integers(0, 10**6, size=n)).astype(np.uint64)
    pay = rng.integers(0, 256, size=int(pls.sum()), dtype=np.uint8)
    if uhl is not None:
        uhl = np.asarray(uhl, dtype=np.uint32)
        uhb = rng.integers(0, 256, size=int(uhl.sum()), dtype=np.uint8)
    else:
        uhb = None
    keep = (ids, ots, pay, pls, uhb, uhl)
    return raw_messages(ids, ots, pay, pls, uhb, uhl), keep


def _encoded(pls, uhl=None, seed=1, stamp=True):
    raw, keep = _mkraw(pls, uhl, seed)
    rc, e, out = O.encode_batch(raw, 3)
    assert rc == 0, e
    if stamp:
        rc, e, h, out = O.stamp_batch(out, 1_000_000 + seed, 1_800_000_000_000_000 + seed)
        assert rc == 0, e
    return np.frombuffer(out, dtype=np.uint8).copy()


_EXPECT = {}


def _expect(rec):
    """The oracle's unpacked arrays of `rec` (computed once per record, never modified)."""
    key = rec.tobytes()
    if key in _EXPECT:
        return _EXPECT[key]
    rc, e, msgs = O.poll_decode(rec, 1)
    assert rc == 0, e
    n = len(msgs)
    pl = np.array([m.payload_length for m in msgs], dtype=np.uint32)
    uh = np.array([m.user_headers_length for m in msgs], dtype=np.uint32)
    x = {
        "ids": np.array([[m.id_lo, m.id_hi] for m in msgs], dtype=np.uint64).reshape(-1),
        "checksums": np.array([m.checksum for m in msgs], dtype=np.uint64),
        "offsets": np.array([m.offset for m in msgs], dtype=np.uint64),
        "timestamps": np.array([m.timestamp for m in msgs], dtype=np.uint64),
        "origin_timestamps": np.array([m.origin_timestamp for m in msgs], dtype=np.uint64),
        "payload_lengths": pl,
        "user_headers_lengths": uh,
        "payload_starts": np.concatenate([[0], np.cumsum(pl, dtype=np.uint64)]).astype(np.uint64),
        "user_headers_starts": np.concatenate([[0], np.cumsum(uh, dtype=np.uint64)]).astype(np.uint64),
        "payloads": np.concatenate([rec[m.payload_pos:m.payload_pos + m.payload_length] for m in msgs]
                                   + [np.zeros(0, np.uint8)]),
        "user_headers": np.concatenate([rec[m.user_headers_pos:m.user_headers_pos + m.user_headers_length]
                                        for m in msgs] + [np.zeros(0, np.uint8)]),
        "n": n,
    }
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _EXPECT[key] = x
    return x


# ------------------------------------------------------------------ harness
class Outs:
    """Every output array as [front guard | capacity | back guard] of 0xA5 bytes."""

    def __init__(self, cap_m, cap_p, cap_u, shift=0, skip=()):
        import torch
        self.cap = (cap_m, cap_p, cap_u)
        self.t, self.front, self.size = {}, {}, {}
        for k in FIELDS:
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


def _place(rec, shift=0):
    buf = np.zeros(rec.size + shift + 16, dtype=np.uint8)
    buf[shift:shift + rec.size] = rec
    return to_device(buf, "cuda:0")[shift:shift + rec.size]


def _enqueue(cx, d_rec, outs, integrity=abi.INTEGRITY_VERIFY, d_cursor=None):
    """decode + unpack on the current stream, no synchronise -> (result tensor, keep-alive)."""
    import torch
    n = d_rec.numel()
    cap = n // 48 + 1
    d_pos = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    d_dec = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device="cuda:0")
    d_res = torch.full((ctypes.sizeof(abi.UnpackResult),), 0xEE, dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    assert cx.decode_device(d_rec.data_ptr(), n, integrity, d_pos.data_ptr(), cap, d_dec.data_ptr(), s) == 0
    assert cx.unpack_device(d_rec.data_ptr(), n, d_pos.data_ptr(), d_dec.data_ptr(), outs.struct(),
                            d_cursor.data_ptr() if d_cursor is not None else None, d_res.data_ptr(), s) == 0
    return d_res, (d_pos, d_dec, d_rec)


def _result(d_res):
    return abi.UnpackResult.from_buffer_copy(to_host(d_res).tobytes())


def _check(got, x, first=0, base_p=0, base_u=0):
    n = x["n"]
    for k in ("checksums", "offsets", "timestamps", "origin_timestamps", "payload_lengths", "user_headers_lengths"):
        if k in got:
            assert np.array_equal(got[k][first:first + n], x[k]), k
    if "ids" in got:
        assert np.array_equal(got["ids"][2 * first:2 * (first + n)], x["ids"])
    if "payload_starts" in got:
        assert np.array_equal(got["payload_starts"][first:first + n + 1], x["payload_starts"] + np.uint64(base_p))
    if "user_headers_starts" in got:
        assert np.array_equal(got["user_headers_starts"][first:first + n + 1],
                              x["user_headers_starts"] + np.uint64(base_u))
    if "payloads" in got:
        assert np.array_equal(got["payloads"][base_p:base_p + x["payloads"].size], x["payloads"])
    if "user_headers" in got:
        assert np.array_equal(got["user_headers"][base_u:base_u + x["user_headers"].size], x["user_headers"])


def _unpack_and_check(cx, rec, integrity=abi.INTEGRITY_VERIFY, dev_shift=0, out_shift=0, slack=0):
    import torch
    x = _expect(rec)
    outs = Outs(x["n"] + slack, x["payloads"].size + slack, x["user_headers"].size + slack, out_shift)
    d_res, keep = _enqueue(cx, _place(rec, dev_shift), outs, integrity)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (0, 0, 0, 0, 0), res.error
    assert (res.count, res.payload_bytes, res.user_headers_bytes, res.first_message) == \
        (x["n"], x["payloads"].size, x["user_headers"].size, 0)
    pl = x["payload_lengths"]
    assert (res.min_payload_length, res.max_payload_length) == (int(pl.min()), int(pl.max()))
    got = outs.host()
    _check(got, x)
    return res, got


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("pl", [0, 1, 15, 16, 17])
def test_single_message_edges(cx, pl):
    _unpack_and_check(cx, _encoded([pl], seed=10 + pl))


def test_empty_payloads_with_user_headers(cx):
    _unpack_and_check(cx, _encoded([0, 0, 0], [5, 5, 5], seed=2))


def _chunk_sharing_record():
    pls = np.arange(64) % 41
    uhl = np.where(np.arange(64) % 3 == 0, 7, 0)
    return _encoded(pls, uhl, seed=3)


def test_messages_sharing_a_destination_chunk(cx):
    _unpack_and_check(cx, _chunk_sharing_record())


def test_more_messages_under_a_span_than_its_staging_holds(cx):
    """3000 messages of 0..8 bytes lie under ONE 32 KiB copy span: past the 1024 starts a
    workgroup stages in LDS, so the copy searches the starts array in place."""
    rng = np.random.default_rng(6)
    _unpack_and_check(cx, _encoded(rng.integers(0, 9, size=3000), rng.integers(0, 2, size=3000) * 3, seed=6))


@pytest.mark.parametrize("n", [255, 256, 257])
def test_tile_boundaries(cx, n):
    _unpack_and_check(cx, O.synth_batch(n, 0, 90, 3, seed=n))


def test_many_tiles_and_spans(cx):
    rec = O.synth_batch(20_000, 0, 600, 7, seed=77)
    res, _ = _unpack_and_check(cx, rec)
    assert res.count == 20_000 and res.payload_bytes > 4 * (32 << 10)  # several tiles, several copy spans


def test_balance_by_bytes(cx):
    rng = np.random.default_rng(5)
    pls = rng.integers(0, 9, size=40)
    pls[20] = 300_000
    pls[39] = 300_000
    _unpack_and_check(cx, _encoded(pls, seed=5))


def test_uniform_payloads_2d(cx):
    rec = O.synth_batch(1000, 1024, 1024, seed=8)
    res, got = _unpack_and_check(cx, rec)
    assert res.min_payload_length == res.max_payload_length == 1024
    x = _expect(rec)
    assert np.array_equal(got["payloads"].reshape(1000, 1024), x["payloads"].reshape(1000, 1024))


def _variable_record():
    return O.synth_batch(700, 0, 300, 9, seed=21)


@pytest.mark.parametrize("dev_shift", [1, 3, 8, 13])
@pytest.mark.parametrize("out_shift", [0, 5, 12])
def test_alignment(cx, dev_shift, out_shift):
    _unpack_and_check(cx, _variable_record(), dev_shift=dev_shift, out_shift=out_shift)


def test_sliced_record(cx):
    rec = O.synth_batch(60, 10, 200, 5, seed=31)
    rc, e, h, _ = O.decode_batch_slice_with(rec, abi.INTEGRITY_VERIFY)
    assert rc == 0, e
    rc, sl, hdr = O.select_slice(rec, abi.LOOKUP_OFFSET, h.base_offset + 7, 20)
    assert rc == 0 and sl.selected and not sl.full_body and sl.matched_messages == 20
    cut = np.concatenate([np.frombuffer(hdr, dtype=np.uint8), rec[256 + sl.start:256 + sl.end]])
    x = _expect(cut)
    assert x["n"] == 20 and x["offsets"][0] == h.base_offset + 7  # the first frame's offset_delta is not 0
    _unpack_and_check(cx, cut, integrity=abi.INTEGRITY_LAYOUT_ONLY)
    _unpack_and_check(cx, cut, integrity=abi.INTEGRITY_VERIFY)


@pytest.mark.parametrize("integrity", [abi.INTEGRITY_VERIFY, abi.INTEGRITY_LAYOUT_ONLY])
def test_both_integrities(cx, integrity):
    _unpack_and_check(cx, _variable_record(), integrity=integrity)
    _unpack_and_check(cx, O.synth_batch(300, 512, 512, seed=4), integrity=integrity)


def test_unwanted_arrays_are_skipped(cx):
    import torch
    rec = _variable_record()
    x = _expect(rec)
    outs = Outs(x["n"], x["payloads"].size, 0, skip=("checksums", "timestamps", "user_headers",
                                                     "user_headers_starts", "ids"))
    d_res, keep = _enqueue(cx, _place(rec), outs)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.kind == 0 and res.count == x["n"] and res.user_headers_bytes == x["user_headers"].size
    _check(outs.host(), x)


# ------------------------------------------------------------------ errors
def _cursor(m=0, p=0, u=0):
    return to_device(np.array([m, p, u, 0], dtype=np.int64), "cuda:0")


def test_gate_failed_decode_writes_nothing(cx):
    import torch
    rec = _variable_record().copy()
    x = _expect(_variable_record())
    rc, e, msgs = O.poll_decode(rec, 1)
    rec[msgs[100].payload_pos + 3] ^= 0x40  # one payload byte
    orc, oe, _, _ = O.decode_batch_slice_with(rec, abi.INTEGRITY_VERIFY)
    assert orc == abi.ERR_INVALID_MESSAGE_CHECKSUM
    outs = Outs(x["n"] + 8, x["payloads"].size + 64, x["user_headers"].size + 64)
    cur = _cursor(2, 7, 3)
    d_res, keep = _enqueue(cx, _place(rec), outs, abi.INTEGRITY_VERIFY, cur)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == oe.astuple()
    assert res.count == 0 and res.payload_bytes == 0 and res.user_headers_bytes == 0
    assert outs.untouched()
    assert to_host(cur).tolist() == [2, 7, 3, 0]
    # the same bytes pass LayoutOnly, and then unpack
    outs = Outs(x["n"], x["payloads"].size, x["user_headers"].size)
    d_res, keep = _enqueue(cx, _place(rec), outs, abi.INTEGRITY_LAYOUT_ONLY)
    torch.cuda.synchronize()
    assert _result(d_res).error.kind == 0 and _result(d_res).count == x["n"]
    outs.host()


@pytest.mark.parametrize("short", ["messages", "payloads", "user_headers"])
def test_capacity(cx, short):
    import torch
    rec = _variable_record()
    x = _expect(rec)
    n, tp, tu = x["n"], x["payloads"].size, x["user_headers"].size
    caps = {"messages": (n - 1, tp, tu), "payloads": (n, tp - 1, tu), "user_headers": (n, tp, tu - 1)}[short]
    outs = Outs(*caps)
    cur = _cursor()
    d_res, keep = _enqueue(cx, _place(rec), outs, abi.INTEGRITY_VERIFY, cur)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (abi.ERR_CAPACITY, 0, n, tp, tu)
    assert res.count == 0
    outs.host()  # guards
    assert to_host(cur).tolist() == [0, 0, 0, 0]


def test_argument_errors(cx):
    import torch
    rec = _variable_record()
    d_rec = _place(rec)
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    ok = abi.UnpackedMessages(1, 1, 1)
    bad = abi.ERR_INVALID_ARGUMENT
    assert cx.unpack_device(None, rec.size, p, p, ok, None, p) == bad
    assert cx.unpack_device(d_rec.data_ptr(), rec.size, p, None, ok, None, p) == bad
    assert cx.unpack_device(d_rec.data_ptr(), rec.size, p, p, ok, None, None) == bad
    assert cx.unpack_device(d_rec.data_ptr(), 255, p, p, ok, None, p) == bad
    no_starts = abi.UnpackedMessages(1, 1, 1)
    no_starts.payloads = p
    assert cx.unpack_device(d_rec.data_ptr(), rec.size, p, p, no_starts, None, p) == bad
    no_starts = abi.UnpackedMessages(1, 1, 1)
    no_starts.user_headers = p
    assert cx.unpack_device(d_rec.data_ptr(), rec.size, p, p, no_starts, None, p) == bad


# ------------------------------------------------------------------ chaining
def test_cursor_chain(cx):
    import torch
    recs = [_variable_record(), _chunk_sharing_record(), O.synth_batch(300, 512, 512, seed=4)]
    xs = [_expect(r) for r in recs]
    outs = Outs(sum(x["n"] for x in xs), sum(x["payloads"].size for x in xs),
                sum(x["user_headers"].size for x in xs))
    cur = _cursor()
    queued = [_enqueue(cx, _place(r), outs, abi.INTEGRITY_VERIFY, cur) for r in recs]
    torch.cuda.synchronize()  # the only one
    got = outs.host()
    first = bp = bu = 0
    for (d_res, keep), x in zip(queued, xs):
        res = _result(d_res)
        assert res.error.kind == 0 and res.count == x["n"] and res.first_message == first
        _check(got, x, first, bp, bu)  # (the starts' entry [first + n] is the next record's entry [first])
        first, bp, bu = first + x["n"], bp + x["payloads"].size, bu + x["user_headers"].size
    assert to_host(cur).tolist() == [first, bp, bu, 0]
    assert got["payload_starts"][first] == bp and got["user_headers_starts"][first] == bu


# ------------------------------------------------------------------ round trip
@pytest.mark.parametrize("n,lo,hi,uh", [(2, 5, 6, True), (100, 64, 4096, False)])
def test_round_trip_with_the_encoder(cx, n, lo, hi, uh):
    import torch
    rng = np.random.default_rng(n)
    pls = rng.integers(lo, hi + 1, size=n)
    uhl = rng.integers(1, 30, size=n) if uh else None
    raw, (ids, ots, pay, pl, uhb, ul) = _mkraw(pls, uhl, seed=40 + n)
    rc, e, wire = O.encode_batch(raw, 0)
    assert rc == 0, e
    rec = np.frombuffer(wire, dtype=np.uint8).copy()
    tp, tu = int(pl.sum()), int(ul.sum()) if uh else 0
    outs = Outs(n, tp, tu)
    d_res, keep = _enqueue(cx, _place(rec), outs)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.kind == 0 and res.count == n
    got = outs.host()
    assert np.array_equal(got["ids"], ids) and np.array_equal(got["origin_timestamps"], ots)
    assert np.array_equal(got["payload_lengths"], pl) and np.array_equal(got["payloads"], pay)
    if uh:
        assert np.array_equal(got["user_headers_lengths"], ul) and np.array_equal(got["user_headers"], uhb)
    else:
        assert not got["user_headers_lengths"].any()
    # the unpacked device arrays ARE an iggy_raw_messages: encoding them gives the record back
    draw = abi.RawMessages(n, outs.ptr("ids"), outs.ptr("origin_timestamps"), outs.ptr("payloads"),
                           outs.ptr("payload_lengths"), outs.ptr("user_headers") if uh else None,
                           outs.ptr("user_headers_lengths"))
    d_out = torch.full((rec.size + 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
    d_er = torch.zeros(ctypes.sizeof(abi.EncodeResult), dtype=torch.uint8, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    assert cx.encode_device(draw, 0, d_out.data_ptr(), rec.size, d_er.data_ptr(), s) == 0
    torch.cuda.synchronize()
    er = abi.EncodeResult.from_buffer_copy(to_host(d_er).tobytes())
    assert er.error.kind == 0 and er.batch_length == rec.size
    assert to_host(d_out)[:rec.size].tobytes() == wire


# ------------------------------------------------------------------ torch_io
def test_torch_io_unpack_record(cx):
    from iggy_amd.codec import CodecError
    from iggy_amd.torch_io import unpack_record
    rec = O.synth_batch(300, 512, 512, seed=4)
    x = _expect(rec)
    r = unpack_record(cx, _place(rec))
    assert r["count"] == 300 and r["first_message"] == 0
    for k in FIELDS:
        want = x[k]
        got = to_host(r[k]).reshape(-1)
        assert got.size * got.itemsize == want.size * want.itemsize, k
        assert got.tobytes() == want.tobytes(), k
    assert tuple(r["payloads_2d"].shape) == (300, 512)
    assert np.array_equal(to_host(r["payloads_2d"]), x["payloads"].reshape(300, 512))
    v = _variable_record()
    rv = unpack_record(cx, _place(v), abi.INTEGRITY_LAYOUT_ONLY)
    assert "payloads_2d" not in rv and to_host(rv["payloads"]).tobytes() == _expect(v)["payloads"].tobytes()
    bad = rec.copy()
    bad[256 + 48 + 5] ^= 1
    _, oe, _, _ = O.decode_batch_slice_with(bad, abi.INTEGRITY_VERIFY)
    with pytest.raises(CodecError) as ei:
        unpack_record(cx, _place(bad))
    assert ei.value.err.astuple() == oe.astuple() and ei.value.rc == abi.ERR_INVALID_MESSAGE_CHECKSUM
