"""GPU tests of the byte copy the unpack, the select and the route share (k_soa_copy,
soa_common.hpp): one record goes through unpack -> select -> route, each stage reading the
arrays the stage before wrote, and every stage's arrays must equal the unpack's byte for
byte.

The expected arrays come from the oracle alone (O.poll_decode and the record's own bytes,
as tests/test_unpack_gpu.py). Every output array sits between 0xA5 guards that must
survive. Integer byte work: every comparison is bit-exact."""
import ctypes
import functools

import numpy as np
import pytest

from iggy_amd import abi
from iggy_amd.torch_io import to_device, to_host
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
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
def _shape(name):
    """-> payload lengths, user-header lengths: the smallest shapes at which the copy takes
    each of its paths."""
    if name == "meet_in_a_chunk":  # 1 + 15 + 17 B: three messages meet inside 16-B chunks
        return [1, 15, 17], [15, 17, 1]
    i = np.arange(300)
    if name == "shared_chunks_across_a_tile":  # 0..40 B, some user headers empty, past the 256-message tile
        return i % 41, np.where(i % 3 == 0, 0, i % 7)
    if name == "in_place_and_across_a_span":
        # 1100 messages of 8 B lie under one 32 KiB span (more than the 1022 it stages: read in
        # place), and one of 40 000 B crosses a span
        return [8] * 1100 + [40_000], [3, 0] * 550 + [21]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _record(name):
    """-> (the record, the oracle's unpacked arrays of it); built once, never modified."""
    from iggy_amd.codec import raw_messages
    pls, uhl = (np.asarray(v, dtype=np.uint32) for v in _shape(name))
    rng = np.random.default_rng(pls.size)
    ids = rng.integers(1, 2**63, size=2 * pls.size, dtype=np.uint64)
    ots = (1_700_000_000_000_000 + rng.integers(0, 10**6, size=pls.size)).astype(np.uint64)
    pay = rng.integers(0, 256, size=int(pls.sum()), dtype=np.uint8)
    uhb = rng.integers(0, 256, size=int(uhl.sum()), dtype=np.uint8)
    rc, e, out = O.encode_batch(raw_messages(ids, ots, pay, pls, uhb, uhl), 3)
    assert rc == 0, e
    rc, e, h, out = O.stamp_batch(out, 1_000_000, 1_800_000_000_000_000)
    assert rc == 0, e
    rec = np.frombuffer(out, dtype=np.uint8).copy()
    rc, e, msgs = O.poll_decode(rec, 1)
    assert rc == 0 and len(msgs) == pls.size, e
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
        "payloads": np.concatenate([rec[m.payload_pos:m.payload_pos + m.payload_length] for m in msgs]),
        "user_headers": np.concatenate([rec[m.user_headers_pos:m.user_headers_pos + m.user_headers_length]
                                        for m in msgs]),
    }
    for v in (rec, *x.values()):
        v.setflags(write=False)
    return rec, x


def _take(x, idx):
    """The arrays of the messages `idx` of x, compacted in that order."""
    idx = np.asarray(idx)
    y = {k: x[k][idx] for k in FIELDS[1:7]}
    y["ids"] = x["ids"].reshape(-1, 2)[idx].reshape(-1)
    for b, s, ln in (("payloads", "payload_starts", "payload_lengths"),
                     ("user_headers", "user_headers_starts", "user_headers_lengths")):
        y[s] = np.concatenate([[0], np.cumsum(y[ln], dtype=np.uint64)]).astype(np.uint64)
        y[b] = np.concatenate([x[b][int(x[s][i]):int(x[s][i + 1])] for i in idx] + [np.zeros(0, np.uint8)])
    return y


# ------------------------------------------------------------------ harness
class Arrays:
    """The eleven arrays at capacities of exactly n messages and p / u bytes, each as
    [front guard | capacity | back guard] of 0xA5; the byte arrays start `shift` bytes past a
    16-B boundary and, with tight, end their tensors (no back guard)."""

    def __init__(self, n, p, u, shift=0, tight=False):
        import torch
        self.cap = (n, p, u)
        self.t, self.front, self.size = {}, {}, {}
        for k in FIELDS:
            size = {"payloads": p, "user_headers": u, "ids": 16 * n}.get(
                k, 4 * n if k in U32 else 8 * (n + 1) if k.endswith("_starts") else 8 * n)
            front = GUARD + (shift if k in BYTES else 0)
            back = 0 if tight and k in BYTES else GUARD
            self.t[k] = torch.full((front + size + back,), FILL, dtype=torch.uint8, device="cuda:0")
            assert self.t[k].data_ptr() % 16 == 0
            self.front[k], self.size[k] = front, size

    def struct(self):
        return abi.UnpackedMessages(*self.cap, *(self.t[k].data_ptr() + self.front[k] for k in FIELDS))

    def check(self, y, stage):
        """Every array equals y's and every guard byte is untouched."""
        for k, t in self.t.items():
            h = to_host(t)
            f, s = self.front[k], self.size[k]
            assert (h[:f] == FILL).all(), f"{stage}: front guard of {k}"
            assert (h[f + s:] == FILL).all(), f"{stage}: back guard of {k}"
            body = h[f:f + s]
            got = body if k in BYTES else body.view(np.uint32 if k in U32 else np.uint64)
            assert np.array_equal(got, y[k]), f"{stage}: {k}"


def _chain(cx, name, shift, last_only=False):
    """unpack -> select -> route (one partition) of the record, queued back to back. The
    select keeps every message, or with last_only the source's last one alone; then the
    source byte arrays of every stage end their tensors."""
    import torch
    rec, x = _record(name)
    n = x["payload_lengths"].size
    y = _take(x, [n - 1]) if last_only else x
    m = y["payload_lengths"].size
    s = torch.cuda.current_stream().cuda_stream

    def result(struct):
        return torch.full((ctypes.sizeof(struct),), 0xEE, dtype=torch.uint8, device="cuda:0")

    d_rec = to_device(rec.copy(), "cuda:0")  # (the record ends its tensor)
    cap = rec.size // 48 + 1
    d_pos = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    d_dec = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device="cuda:0")
    d_un, d_sel, d_rt = result(abi.UnpackResult), result(abi.SelectResult), result(abi.RouteResult)
    a = Arrays(n, x["payloads"].size, x["user_headers"].size, shift, tight=last_only)
    b = Arrays(m, y["payloads"].size, y["user_headers"].size, shift, tight=last_only)
    c = Arrays(m, y["payloads"].size, y["user_headers"].size, shift)
    assert cx.decode_device(d_rec.data_ptr(), rec.size, abi.INTEGRITY_VERIFY, d_pos.data_ptr(), cap,
                            d_dec.data_ptr(), s) == 0
    assert cx.unpack_device(d_rec.data_ptr(), rec.size, d_pos.data_ptr(), d_dec.data_ptr(), a.struct(), None,
                            d_un.data_ptr(), s) == 0
    d_cnt = to_device(np.array([n], dtype=np.int64), "cuda:0")
    d_mask = to_device((np.arange(n) == n - 1).astype(np.uint8), "cuda:0") if last_only else None
    spec = abi.SelectSpec.make([], d_mask.data_ptr() if last_only else None)
    assert cx.select_messages_device(a.struct(), d_cnt.data_ptr(), spec, b.struct(), None, None, d_sel.data_ptr(),
                                     s) == 0
    d_first = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    assert cx.route_messages_device(b.struct(), d_sel.data_ptr() + abi.SelectResult.count.offset,
                                    abi.RouteSpec.make(1, abi.ROUTE_KEY_ID), c.struct(), d_first.data_ptr(), None,
                                    None, None, None, d_rt.data_ptr(), s) == 0
    torch.cuda.synchronize()
    un = abi.UnpackResult.from_buffer_copy(to_host(d_un).tobytes())
    sel = abi.SelectResult.from_buffer_copy(to_host(d_sel).tobytes())
    rt = abi.RouteResult.from_buffer_copy(to_host(d_rt).tobytes())
    assert un.error.astuple() == sel.error.astuple() == rt.error.astuple() == (0, 0, 0, 0, 0)
    assert (un.count, sel.examined, sel.count, rt.examined, rt.count) == (n, n, m, m, m)
    assert (un.payload_bytes, un.user_headers_bytes) == (x["payloads"].size, x["user_headers"].size)
    for r in (sel, rt):
        assert (r.payload_bytes, r.user_headers_bytes) == (y["payloads"].size, y["user_headers"].size)
    assert to_host(d_first).tolist() == [0, m]
    a.check(x, "unpack")
    b.check(y, "select")
    c.check(y, "route")


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("shift", [0, 1, 15])
@pytest.mark.parametrize("name", ["meet_in_a_chunk", "shared_chunks_across_a_tile", "in_place_and_across_a_span"])
def test_three_stages_agree(cx, name, shift):
    _chain(cx, name, shift)


def test_last_message_at_the_end_of_every_source(cx):
    """The select keeps the source's last message alone and the route routes it: each
    stage's only bytes end its source (the record, the unpacked arrays, the selected
    arrays), which ends its tensor, so a 16-B load of a boundary piece must stay inside the
    bound of each of the three sources."""
    _chain(cx, "shared_chunks_across_a_tile", 0, last_only=True)
    _chain(cx, "meet_in_a_chunk", 1, last_only=True)
