"""GPU tests of the device user-header validation and key columns
(iggy_codec_user_headers_device / _arrays_device, user_headers.hip).

Expected values come from tests/user_headers_ref.py alone (the plain-Python restatement of
the reference, pinned by its own unit-test vectors on the CPU). Records are built with
O.encode_batch from TLV bytes assembled here; the arrays form runs over the oracle-derived
user_headers / starts (O.poll_decode). Every output array sits between 0xA5 guards that
must survive every case, errors included, and nothing past `count` is written. Integer
byte work: every comparison is bit-exact."""
import ctypes
import random
import struct

import numpy as np
import pytest

import user_headers_ref as R
from iggy_amd import abi
from iggy_amd.torch_io import to_device, to_host
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
NONE = 2**64 - 1
STAGE_MAX = 4096  # headers up to this many bytes are staged in LDS, longer ones walked in place
COLS = (("value_kinds", 1), ("value_lengths", 1), ("value_pos", 4), ("values16", 16))


@pytest.fixture(scope="module")
def cx():
    from iggy_amd.codec import Codec
    c = Codec(0)
    yield c
    c.close()


# ------------------------------------------------------------------ records and expectations
def _record(headers, seed=1, payload=None):
    """A stamped record whose message i carries headers[i] (payload lengths vary unless given)."""
    from iggy_amd.codec import raw_messages
    rng = np.random.default_rng(seed)
    n = len(headers)
    pls = (rng.integers(0, 70, size=n) if payload is None else np.full(n, payload)).astype(np.uint32)
    ids = rng.integers(1, 2**63, size=2 * n, dtype=np.uint64)
    ots = (1_700_000_000_000_000 + rng.integers(0, 10**6, size=n)).astype(np.uint64)
    pay = rng.integers(0, 256, size=int(pls.sum()), dtype=np.uint8)
    uhl = np.array([len(h) for h in headers], dtype=np.uint32)
    uhb = np.frombuffer(b"".join(headers), dtype=np.uint8).copy()
    raw = raw_messages(ids, ots, pay, pls, uhb if uhb.size else None, uhl if uhb.size else None)
    rc, e, out = O.encode_batch(raw, 3)
    assert rc == 0, e
    rc, e, h, out = O.stamp_batch(out, 1_000_000 + seed, 1_800_000_000_000_000 + seed)
    assert rc == 0, e
    return np.frombuffer(out, dtype=np.uint8).copy()


def _arrays_of(rec):
    """The oracle-derived user_headers blob and starts of a record."""
    rc, e, msgs = O.poll_decode(rec, 1)
    assert rc == 0, e
    parts = [rec[m.user_headers_pos:m.user_headers_pos + m.user_headers_length] for m in msgs]
    starts = np.concatenate([[0], np.cumsum([p.size for p in parts], dtype=np.uint64)]).astype(np.uint64)
    return np.concatenate(parts + [np.zeros(0, np.uint8)]), starts


def _expect(headers, keys):
    """The restatement's columns for these messages and keys (computed once per case)."""
    n = len(headers)
    dec = [R.decode(h) for h in headers]
    x = {
        "n": n,
        "status": np.array([d[0] for d in dec], dtype=np.uint32).reshape(n, 4),
        "pairs": np.array([d[1] for d in dec], dtype=np.uint32),
        "with_headers": sum(1 for h in headers if len(h)),
        "invalid": sum(1 for d in dec if d[0] != R.STATUS_OK),
        "first_invalid": next((i for i, d in enumerate(dec) if d[0] != R.STATUS_OK), NONE),
        "cols": [], "found": [],
    }
    for key in keys:
        rows = [R.lookup(d, key) for d in dec]
        x["cols"].append({
            "value_kinds": np.array([r[0] for r in rows], dtype=np.uint8),
            "value_pos": np.array([r[1] for r in rows], dtype=np.uint32),
            "value_lengths": np.array([r[2] for r in rows], dtype=np.uint8),
            "values16": np.frombuffer(b"".join(r[3] for r in rows), dtype=np.uint8).reshape(n, 16),
        })
        x["found"].append(sum(1 for r in rows if r[0]))
    return x


# ------------------------------------------------------------------ harness
class Outs:
    """Every output array as [front guard | capacity | back guard] of 0xA5 bytes; the u8
    arrays (and with them every array) can be based at an odd address (shift)."""

    def __init__(self, cap, keys, shift=0, skip=()):
        import torch
        self.cap, self.keys, self.shift = cap, keys, shift
        self.t, self.size = {}, {}
        names = [("status", 16), ("pairs", 4)] + [(f"{f}{k}", w) for k in range(len(keys)) for f, w in COLS]
        for name, width in names:
            if name in skip:
                continue
            front = GUARD + (shift if width in (1, 16) else 0)
            self.t[name] = (torch.full((front + width * cap + GUARD,), FILL, dtype=torch.uint8, device="cuda:0"), front)
            self.size[name] = width * cap

    def ptr(self, name):
        return self.t[name][0].data_ptr() + self.t[name][1] if name in self.t else None

    def struct(self, cap=None):
        q = abi.HeaderColumns()
        q.cap_messages, q.nkeys = self.cap if cap is None else cap, len(self.keys)
        q.status, q.pairs = self.ptr("status"), self.ptr("pairs")
        for k, key in enumerate(self.keys):
            q.keys[k] = abi.HeaderKey.make(*key)
            q.columns[k] = abi.HeaderColumn(*(self.ptr(f"{f}{k}") for f, _ in COLS))
        return q

    def host(self):
        """-> {name: the capacity region as bytes}; asserts the guards."""
        out = {}
        for name, (t, front) in self.t.items():
            h = to_host(t)
            s = self.size[name]
            assert (h[:front] == FILL).all(), f"front guard of {name}"
            assert (h[front + s:] == FILL).all(), f"back guard of {name}"
            out[name] = h[front:front + s].copy()
        return out

    def untouched(self):
        return all((to_host(t) == FILL).all() for t, _ in self.t.values())


def _place(a, shift=0):
    buf = np.zeros(a.size + shift + 16, dtype=np.uint8)
    buf[shift:shift + a.size] = a
    return to_device(buf, "cuda:0")[shift:shift + a.size]


def _result(d_res):
    return abi.HeaderColumnsResult.from_buffer_copy(to_host(d_res).tobytes())


def _new_result():
    import torch
    return torch.full((ctypes.sizeof(abi.HeaderColumnsResult),), 0xEE, dtype=torch.uint8, device="cuda:0")


def _enqueue_record(cx, d_rec, q, integrity=abi.INTEGRITY_VERIFY):
    """decode + user headers on the current stream, no synchronise."""
    import torch
    n = d_rec.numel()
    cap = n // 48 + 1
    d_pos = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    d_dec = torch.zeros(ctypes.sizeof(abi.DecodeResult), dtype=torch.uint8, device="cuda:0")
    d_res = _new_result()
    s = torch.cuda.current_stream().cuda_stream
    assert cx.decode_device(d_rec.data_ptr(), n, integrity, d_pos.data_ptr(), cap, d_dec.data_ptr(), s) == 0
    assert cx.user_headers_device(d_rec.data_ptr(), n, d_pos.data_ptr(), d_dec.data_ptr(), q, d_res.data_ptr(), s) == 0
    return d_res, (d_pos, d_dec, d_rec)


def _enqueue_arrays(cx, blob, starts, count, q, shift=0, hint=None):
    import torch
    d_blob = _place(blob if blob.size else np.zeros(1, np.uint8), shift)
    d_starts = to_device(starts.view(np.int64), "cuda:0")
    d_count = to_device(np.array([count, 99, 99, 99], dtype=np.int64), "cuda:0")
    d_res = _new_result()
    s = torch.cuda.current_stream().cuda_stream
    assert cx.user_headers_arrays_device(d_blob.data_ptr(), d_starts.data_ptr(), d_count.data_ptr(),
                                         count if hint is None else hint, q, d_res.data_ptr(), s) == 0
    return d_res, (d_blob, d_starts, d_count)


def _check(res, got, x, keys):
    n = x["n"]
    assert res.error.astuple() == (0, 0, 0, 0, 0), res.error
    assert (res.count, res.with_headers, res.invalid_messages, res.first_invalid) == \
        (n, x["with_headers"], x["invalid"], x["first_invalid"])
    assert [res.found[k] for k in range(16)] == x["found"] + [0] * (16 - len(keys))
    if "status" in got:
        st = got["status"].view(np.uint32).reshape(-1, 4)
        bad = np.nonzero((st[:n] != x["status"]).any(axis=1))[0]
        assert bad.size == 0, (int(bad[0]), st[bad[0]].tolist(), x["status"][bad[0]].tolist())
    if "pairs" in got:
        assert np.array_equal(got["pairs"].view(np.uint32)[:n], x["pairs"])
    for k in range(len(keys)):
        for f, w in COLS:
            name = f"{f}{k}"
            if name not in got:
                continue
            g = got[name]
            g = g.view(np.uint32) if f == "value_pos" else g.reshape(-1, 16) if f == "values16" else g
            bad = np.nonzero(g[:n] != x["cols"][k][f])[0]
            assert bad.size == 0, (name, int(bad[0]), g[bad[0]].tolist(), x["cols"][k][f][bad[0]].tolist())
    # nothing outside [0, count) of any array
    for name, g in got.items():
        w = 16 if name == "status" or name.startswith("values16") else 4 if name == "pairs" or name.startswith("value_pos") else 1
        assert (g[w * n:] == FILL).all(), f"{name} written past count"


def _run(cx, headers, keys, form="record", rec_shift=0, col_shift=0, slack=3, skip=(), seed=1, payload=None):
    import torch
    x = _expect(headers, keys)
    outs = Outs(x["n"] + slack, keys, col_shift, skip)
    rec = _record(headers, seed, payload)
    if form == "record":
        d_res, keep = _enqueue_record(cx, _place(rec, rec_shift), outs.struct())
    else:
        blob, starts = _arrays_of(rec)
        assert blob.tobytes() == b"".join(headers)
        d_res, keep = _enqueue_arrays(cx, blob, starts, x["n"], outs.struct(), rec_shift)
    torch.cuda.synchronize()
    res = _result(d_res)
    _check(res, outs.host(), x, keys)
    return res, x


FORMS = ["record", "arrays"]
KEYS2 = [(2, b"route"), (7, struct.pack("<q", 5))]


def _small_headers(n, seed):
    """2 to 4 valid pairs per message, keys from a small pool"""
    rng = random.Random(seed)
    pool = [(2, b"route"), (7, struct.pack("<q", 5)), (2, b"other"), (1, b"route"), (3, b"\x01")]
    out = []
    for _ in range(n):
        pairs = []
        for key in rng.sample(pool, rng.randint(2, 4)):
            vk = rng.choice([2, 7, 6, 13, 3])
            size = R.EXPECTED_SIZE[vk]
            pairs.append(R.pair(*key, vk, rng.randbytes(size if size is not None else rng.randint(1, 20))))
        out.append(b"".join(pairs))
    return out


# ------------------------------------------------------------------ counts, empties, alignment
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4096])
def test_counts(cx, n, form):
    _run(cx, _small_headers(n, n), KEYS2, form, seed=n)


@pytest.mark.parametrize("every_other", [False, True])
def test_no_headers(cx, every_other):
    hs = _small_headers(300, 7)
    hs = [h if every_other and i % 2 else b"" for i, h in enumerate(hs)]
    res, x = _run(cx, hs, KEYS2, seed=8)
    assert res.with_headers == (150 if every_other else 0) and res.invalid_messages == 0


@pytest.mark.parametrize("form,shift", [("record", 1), ("record", 7), ("record", 15), ("arrays", 1), ("arrays", 15)])
def test_unaligned_views(cx, form, shift):
    _run(cx, _small_headers(300, 11), KEYS2, form, rec_shift=shift, col_shift=shift | 1, seed=11)


# ------------------------------------------------------------------ the catalogue of verdicts and lookups
K = (2, b"k")
BIGKEY = (2, b"K" * 255)
CAT_KEYS = [K, (1, b"k"), (2, b"ke"), (2, b"kf"), BIGKEY, (6, struct.pack("<i", 7)), K, (2, b"big")] + \
           [(2, b"pad%d" % i) for i in range(8)]


def _catalogue():
    fixed = [k for k in range(1, 16) if R.EXPECTED_SIZE[k] is not None]
    two = R.pair(2, b"ke", 7, bytes(range(8))) + R.pair(1, b"k", 2, b"vv")
    hs = []
    # kinds: every kind as value at its exact size; every fixed kind one byte short and one long
    for kind in range(1, 16):
        hs.append(R.pair(*K, kind, bytes(range(1, 1 + (R.EXPECTED_SIZE[kind] or 9)))))
    for kind in fixed:
        hs.append(R.pair(*K, kind, bytes(R.EXPECTED_SIZE[kind] - 1)))
        hs.append(R.pair(*K, kind, bytes(R.EXPECTED_SIZE[kind] + 1)))
    # domain errors
    hs.append(R.pair(6, b"abc", 2, b"v"))
    for kk, vk in ((16, 2), (255, 2), (2, 16), (2, 255), (16, 255), (255, 16)):
        hs.append(R.pair(*K, 2, b"fine") + R.pair(kk, b"k", vk, b"v"))
    hs.append(R.pair(6, b"abc", 16, b"v"))  # the kind error wins over the key size
    # structural errors: every proper prefix of a valid two-pair buffer, a trailing byte,
    # kind 0 at either position, lengths 0 / 256 / 0xFFFFFFFF
    hs += [two[:i] for i in range(1, len(two))]
    hs.append(two + b"\x07")
    hs.append(R.tlv(0, b"k") + R.tlv(2, b"v"))
    hs.append(R.tlv(2, b"k") + R.tlv(0, b"v"))
    for length in (0, 256, 0xFFFFFFFF):
        hs.append(R.tlv(2, b"k") + R.tlv(2, b"v" * 300, length))
        hs.append(R.tlv(2, b"k" * 300, length) + R.tlv(2, b"v"))
    # precedence: structural (pair 2) over domain (pair 0); the first of two domain errors
    hs.append(R.pair(16, b"k", 2, b"v") + R.pair(*K, 2, b"v") + R.tlv(2, b"x") + R.tlv(2, b"y", 0))
    hs.append(R.pair(*K, 5, b"abc") + R.pair(6, b"ab", 2, b"v"))
    hs.append(R.pair(6, b"ab", 2, b"v") + R.pair(*K, 5, b"abc"))
    # lookup
    hs.append(R.pair(*K, 2, b"first") + R.pair(2, b"x", 2, b"y") + R.pair(*K, 2, b"second"))
    hs.append(R.pair(*K, 6, struct.pack("<i", -2)) + R.pair(*K, 2, b"now a string"))
    hs.append(R.pair(2, b"k", 2, b"string") + R.pair(1, b"k", 1, b"raw"))
    hs.append(R.pair(2, b"ke", 2, b"long") + R.pair(2, b"k", 2, b"short") + R.pair(2, b"kf", 2, b"other"))
    hs.append(R.pair(2, b"kf", 3, b"\x01"))
    hs.append(R.pair(*BIGKEY, 1, bytes(range(255))) + R.pair(2, b"K" * 254 + b"J", 2, b"near miss"))
    hs.append(R.pair(2, b"big", 2, b"0123456789abcdefG") + R.pair(6, struct.pack("<i", 7), 12, struct.pack("<Q", 2**63 + 5)))
    hs.append(two)
    return hs


@pytest.mark.parametrize("form", FORMS)
def test_catalogue_with_16_keys(cx, form):
    hs = _catalogue()
    res, x = _run(cx, hs, CAT_KEYS, form, seed=21)
    kinds = {tuple(s[:2]) if s[0] != 29 else (29, 0) for s in x["status"].tolist()}
    assert {(0, 0), (1, 0), (2, 11), (2, 12), (2, 13), (27, 0), (28, 0), (29, 0)} <= kinds  # not vacuous
    assert x["found"][0] == x["found"][6] > 15 and min(x["found"][:8]) > 0  # a key given twice: equal columns
    assert x["cols"][7]["value_lengths"].max() == 17 and x["cols"][4]["value_lengths"].max() == 255


def test_zero_request_keys(cx):
    res, x = _run(cx, _catalogue(), [], seed=22)
    assert res.invalid_messages > 40


# ------------------------------------------------------------------ the long path
def _filled(nbytes, tail=b""):
    """valid headers of exactly nbytes ending in `tail`"""
    parts, rem = [], nbytes - len(tail)
    while rem:
        size = min(rem, 266)
        if 0 < rem - size < 12:
            size -= 12
        assert size >= 12
        parts.append(R.pair(2, b"f", 1, bytes(size - 11)))
        rem -= size
    out = b"".join(parts) + tail
    assert len(out) == nbytes and R.decode(out)[0] == R.STATUS_OK
    return out


NEEDLE = (2, b"needle1234")


def _long_case(broken):
    tail = R.pair(*NEEDLE, 7, struct.pack("<q", -77))
    big = b"".join([R.pair(2, b"a", 2, b"v")] * 8331) + tail
    assert len(big) == 100_000 and R.decode(big)[1] == 8332
    if broken:  # the last value's length field = 0
        big = big[:-12] + struct.pack("<I", 0) + big[-8:]
        assert R.decode(big)[0] == (R.ERR_VALIDATION, R.V_HEADER_FIELD_LENGTH, 100_000 - 12, 0)
    hs = _small_headers(300, 31)
    hs.insert(137, big)
    hs[5] = R.pair(*NEEDLE, 2, b"small too")
    return hs


@pytest.mark.parametrize("broken", [False, True])
def test_one_long_message_among_small_ones(cx, broken):
    res, x = _run(cx, _long_case(broken), [NEEDLE, (2, b"route")], seed=32)
    assert res.found[0] == (1 if broken else 2) and res.invalid_messages == int(broken)
    assert res.first_invalid == (137 if broken else NONE)


@pytest.mark.parametrize("form", FORMS)
def test_staging_threshold(cx, form):
    tail = R.pair(*NEEDLE, 13, bytes(range(16)))
    hs = _small_headers(70, 41)
    for j, d in enumerate((-1, 0, 1, 2000)):
        hs[3 + 20 * j] = _filled(STAGE_MAX + d, tail)
    hs[66] = _filled(STAGE_MAX + 1, tail)[:-3]  # a long one that ends early
    # 70 messages hold more than one 32 KiB stage round of headers when many are large
    hs[10:14] = [_filled(STAGE_MAX - 7 * j, tail) for j in range(4)]
    hs[44:50] = [_filled(3000 + j, tail) for j in range(6)]
    res, x = _run(cx, hs, [NEEDLE, (2, b"route")], form, seed=42)
    assert res.found[0] == 14 and res.invalid_messages == 1 and res.first_invalid == 66


# ------------------------------------------------------------------ optional arrays, gate, capacity, arguments
@pytest.mark.parametrize("skip", ["status", "pairs", "value_kinds0", "value_lengths1", "value_pos0", "values161"])
def test_each_optional_array_null(cx, skip):
    _run(cx, _catalogue(), KEYS2 + [K], skip=(skip,), seed=51)


def test_all_arrays_null_counts_only(cx):
    names = ["status", "pairs"] + [f"{f}{k}" for k in range(2) for f, _ in COLS]
    _run(cx, _catalogue(), [K, (1, b"k")], skip=names, seed=52)


def test_gate_failed_decode_writes_nothing(cx):
    import torch
    hs = _small_headers(300, 61)
    rec = _record(hs, 61, payload=40)
    rc, e, msgs = O.poll_decode(rec, 1)
    rec[msgs[100].payload_pos + 3] ^= 0x40  # one payload byte
    orc, oe, _, _ = O.decode_batch_slice_with(rec, abi.INTEGRITY_VERIFY)
    assert orc == abi.ERR_INVALID_MESSAGE_CHECKSUM
    outs = Outs(310, KEYS2)
    d_res, keep = _enqueue_record(cx, _place(rec), outs.struct(), abi.INTEGRITY_VERIFY)
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == oe.astuple()
    assert (res.count, res.with_headers, res.invalid_messages, res.first_invalid) == (0, 0, 0, NONE)
    assert not any(res.found) and outs.untouched()
    # the same bytes pass LayoutOnly, and then the headers are read
    outs = Outs(300, KEYS2)
    d_res, keep = _enqueue_record(cx, _place(rec), outs.struct(), abi.INTEGRITY_LAYOUT_ONLY)
    torch.cuda.synchronize()
    _check(_result(d_res), outs.host(), _expect(hs, KEYS2), KEYS2)


@pytest.mark.parametrize("form", FORMS)
def test_capacity(cx, form):
    import torch
    hs = _small_headers(300, 71)
    rec = _record(hs, 71)
    outs = Outs(299, KEYS2)
    if form == "record":
        d_res, keep = _enqueue_record(cx, _place(rec), outs.struct())
    else:
        d_res, keep = _enqueue_arrays(cx, *_arrays_of(rec), 300, outs.struct())
    torch.cuda.synchronize()
    res = _result(d_res)
    assert res.error.astuple() == (abi.ERR_CAPACITY, 0, 300, 0, 0)
    assert (res.count, res.with_headers, res.invalid_messages, res.first_invalid) == (0, 0, 0, NONE)
    assert not any(res.found) and outs.untouched()


def test_argument_errors_with_a_context(cx):
    import torch
    from test_user_headers_cpu import malformed_requests
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr()
    bad = abi.ERR_INVALID_ARGUMENT
    ok = Outs(4, KEYS2).struct()
    assert cx.user_headers_device(None, 512, p, p, ok, p) == bad
    assert cx.user_headers_device(p, 512, None, p, ok, p) == bad
    assert cx.user_headers_device(p, 512, p, None, ok, p) == bad
    assert cx.user_headers_device(p, 512, p, p, ok, None) == bad
    assert cx.user_headers_device(p, 255, p, p, ok, p) == bad
    assert cx.user_headers_arrays_device(p, None, p, 4, ok, p) == bad
    assert cx.user_headers_arrays_device(p, p, None, 4, ok, p) == bad
    assert cx.user_headers_arrays_device(p, p, p, 4, ok, None) == bad
    for name, q in malformed_requests().items():
        assert cx.user_headers_device(p, 512, p, p, q, p) == bad, name
        assert cx.user_headers_arrays_device(p, p, p, 4, q, p) == bad, name


def test_1024_key_bytes_are_accepted(cx):
    keys = [(2, bytes([65 + i]) * 255) for i in range(4)] + [(2, b"tail")]
    hs = [R.pair(*keys[i % 5], 2, b"v%d" % i) for i in range(40)]
    res, x = _run(cx, hs, keys, seed=81)
    assert x["found"] == [8] * 5


# ------------------------------------------------------------------ chained unpack -> arrays form
def test_arrays_form_over_a_cursor_chain(cx):
    import torch
    from iggy_amd.torch_io import unpack_record
    lists = [_small_headers(300, 91), _catalogue(), _small_headers(70, 92)]
    keys = CAT_KEYS[:4] + KEYS2
    cursor = to_device(np.zeros(4, dtype=np.int64), "cuda:0")
    parts = [unpack_record(cx, _place(_record(hs, 90 + j)), cursor=cursor) for j, hs in enumerate(lists)]
    uh = torch.cat([p["user_headers"] for p in parts])
    starts = torch.cat([p["user_headers_starts"][:-1] for p in parts] + [parts[-1]["user_headers_starts"][-1:]])
    allh = [h for hs in lists for h in hs]
    x = _expect(allh, keys)  # (the restatement runs message by message: record by record)
    assert to_host(uh).tobytes() == b"".join(allh) and starts.numel() == x["n"] + 1
    outs = Outs(x["n"] + 2, keys)
    d_res = _new_result()
    s = torch.cuda.current_stream().cuda_stream
    assert cx.user_headers_arrays_device(uh.data_ptr(), starts.data_ptr(), cursor.data_ptr(), x["n"],
                                         outs.struct(), d_res.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert int(to_host(cursor)[0]) == x["n"]
    _check(_result(d_res), outs.host(), x, keys)


# ------------------------------------------------------------------ seeded mix
POOL = [(2, b"route"), (2, b"tenant"), (1, b"route"), (6, struct.pack("<i", 1)), (7, struct.pack("<q", 2)),
        (2, b"trace-id"), (3, b"\x01"), (13, bytes(range(16)))]


def _mix(n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        r = rng.random()
        if r < 0.1:
            out.append(rng.randbytes(rng.randint(1, 60)))
            continue
        pairs = []
        for _ in range(rng.randint(1, 12)):
            vk = rng.randint(1, 15)
            size = R.EXPECTED_SIZE[vk]
            pairs.append([*rng.choice(POOL), vk, rng.randbytes(size if size is not None else rng.randint(1, 40))])
        if 0.1 <= r < 0.3:  # a domain error: an unknown kind, or a fixed-size value of another size
            p = rng.choice(pairs)
            if rng.random() < 0.5:
                p[rng.choice([0, 2])] = rng.choice([16, 77, 255])
            else:
                p[2], p[3] = rng.choice([5, 6, 7, 8]), rng.randbytes(rng.choice([1, 3, 5, 9]))
        buf = b"".join(R.pair(*p) for p in pairs)
        if 0.3 <= r < 0.5:  # a structural error: cut short, or one length / kind byte cleared
            if rng.random() < 0.5:
                buf = buf[:rng.randint(1, len(buf) - 1)]
            else:
                buf = buf[:1] + b"\x00" + buf[2:] if rng.random() < 0.5 else b"\x00" + buf[1:]
        elif 0.5 <= r < 0.6:  # any one byte
            i = rng.randrange(len(buf))
            buf = buf[:i] + bytes([rng.randrange(256)]) + buf[i + 1:]
        out.append(buf)
    return out


def test_seeded_mix(cx):
    hs = _mix(2048, 4242)
    keys = [POOL[0], POOL[3], POOL[4], POOL[7]]
    x = _expect(hs, keys)
    kinds = x["status"][:, 0]
    assert (kinds == 0).sum() * 3 >= 2048                      # at least one third OK
    assert np.isin(kinds, (1, 2)).sum() * 10 >= 2048           # at least one tenth structural
    assert np.isin(kinds, (27, 28, 29)).sum() * 10 >= 2048     # at least one tenth domain
    assert min(x["found"]) >= 100
    _run(cx, hs, keys, seed=43)


# ------------------------------------------------------------------ torch_io
def test_torch_io_header_columns(cx):
    import torch
    from iggy_amd.codec import CodecError
    from iggy_amd.torch_io import header_columns
    rng = random.Random(5)
    vals = [rng.randrange(-2**63, 2**63) for _ in range(90)]
    hs = [R.pair(2, b"seq", 7, struct.pack("<q", v)) + R.pair(2, b"route", 2, b"r%d" % i) if i % 9 else b""
          for i, v in enumerate(vals)]
    hs[50] = hs[50][:-1]
    keys = [(abi.KIND_STRING, b"seq"), (abi.KIND_STRING, b"route")]
    x = _expect(hs, keys)
    rec = _record(hs, 5, payload=40)
    r = header_columns(cx, _place(rec), keys)
    assert (r["count"], r["with_headers"], r["invalid_messages"], r["first_invalid"]) == (90, 80, 1, 50)
    assert r["found"] == x["found"] == [79, 79]
    assert np.array_equal(to_host(r["status"]).view(np.uint32), x["status"])
    assert np.array_equal(to_host(r["pairs"]).view(np.uint32), x["pairs"])
    for k in range(2):
        col = r["columns"][k]
        assert tuple(col["values16"].shape) == (90, 16)
        for f, _ in COLS:
            assert np.array_equal(to_host(col[f]).view(x["cols"][k][f].dtype), x["cols"][k][f]), f
    seq = r["columns"][0]["values16"].view(torch.int64)[:, 0]  # the documented idiom
    want = np.array([v if x["cols"][0]["value_kinds"][i] else 0 for i, v in enumerate(vals)], dtype=np.int64)
    assert np.array_equal(to_host(seq), want)
    assert np.array_equal(to_host(seq), x["cols"][0]["values16"].copy().view(np.int64)[:, 0])
    bad = rec.copy()
    rc, e, msgs = O.poll_decode(rec, 1)
    bad[msgs[1].payload_pos] ^= 1
    with pytest.raises(CodecError) as ei:
        header_columns(cx, _place(bad), keys)
    assert ei.value.rc == abi.ERR_INVALID_MESSAGE_CHECKSUM
    assert header_columns(cx, _place(bad), keys, abi.INTEGRITY_LAYOUT_ONLY)["count"] == 90
