"""The route's C ABI, hash and partition rule without a GPU: XXH32 (the tests' restatement
and the library's iggy_xxh32) against tests/golden/xxh32_vectors.json (libxxhash 0.8.2),
the host twin (iggy_route_partitions_host, route.cpp, which shares route_key.hpp and
xxh32.hpp with the device kernel) against the plain-Python restatement (tests/route_ref.py)
for the four key sources, the mask and the drop rules, every synchronous refusal, the
exports and the ctypes mirrors against include/iggy_codec.h."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import route_ref as R
import route_util as RU
import select_util as U
from iggy_amd import abi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iggy_codec.h")
BAD = abi.ERR_INVALID_ARGUMENT


def _ptr(a):
    return a.ctypes.data


def _twin(src, count, spec, cap=None):
    return codec.route_partitions_host(U.src_struct(src, count if cap is None else cap, _ptr), count,
                                       RU.abi_spec(spec, _ptr))


# ------------------------------------------------------------------ the hash
def test_vectors_cover_what_the_contract_names():
    v = RU.vectors()
    assert (b"", 0, 0x02CC5D05) in v and (b"abc", 0, 0x32D153FF) in v
    for seed in (0, 0x9E3779B1):
        lengths = {len(d) for d, s, _ in v if s == seed}
        assert set(range(49)) | {63, 64, 65, 127, 128, 254, 255, 256, 1000} <= lengths


def test_restatement_against_the_vectors():
    for data, seed, want in RU.vectors():
        assert R.xxh32(data, seed) == want, (len(data), seed)


def test_library_xxh32_against_the_vectors():
    for data, seed, want in RU.vectors():
        assert codec.xxh32(data, seed) == want, (len(data), seed)
    # at every alignment of the first byte
    data, _, _ = max(RU.vectors(), key=lambda v: len(v[0]))
    buf = np.zeros(len(data) + 16, np.uint8)
    for k in range(16):
        buf[k:k + 40] = np.frombuffer(data[:40], np.uint8)
        assert codec.lib().iggy_xxh32(buf.ctypes.data + k, 40, 0) == R.xxh32(data[:40])


# ------------------------------------------------------------------ exports, mirrors
def test_library_exports_the_entry_points():
    for name in ("iggy_codec_route_messages_device", "iggy_xxh32", "iggy_route_partitions_host"):
        assert name in codec.exported_symbols()
        assert hasattr(codec.lib(), name)


PAIRS = {"RouteSpec": "iggy_route_spec", "RouteResult": "iggy_route_result"}
CONSTANTS = {"IGGY_ROUTE_MAX_PARTITIONS": abi.ROUTE_MAX_PARTITIONS, "IGGY_ROUTE_DROP": abi.ROUTE_DROP,
             "IGGY_ROUTE_KEY_ID": abi.ROUTE_KEY_ID, "IGGY_ROUTE_KEY_HEADER": abi.ROUTE_KEY_HEADER,
             "IGGY_ROUTE_KEY_BYTES": abi.ROUTE_KEY_BYTES, "IGGY_ROUTE_KEY_PARTITION": abi.ROUTE_KEY_PARTITION,
             "IGGY_CODEC_ABI_VERSION": 1}


@pytest.fixture(scope="module")
def c_layout():
    cc = shutil.which("gcc")
    if not cc:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for name, cname in PAIRS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in getattr(abi, name)._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    for name in CONSTANTS:
        lines.append(f'printf("const {name} %u\\n", (unsigned){name});')
    lines += ["return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run([cc, "-std=c11", "-o", exe, src], check=True, capture_output=True)
        text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in text.splitlines():
        cname, what, val = ln.split()
        got[(cname, what)] = int(val)
    return got


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_mirror_matches_header(name, c_layout):
    cls, cname = getattr(abi, name), PAIRS[name]
    assert ctypes.sizeof(cls) == c_layout[(cname, "size")] == 80, cname
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == c_layout[(cname, f)], (cname, f)


def test_constants_match_header(c_layout):
    for name, value in CONSTANTS.items():
        assert c_layout[("const", name)] == value, name
    assert (R.KEY_ID, R.KEY_HEADER, R.KEY_BYTES, R.KEY_PARTITION, R.DROP) == \
        (abi.ROUTE_KEY_ID, abi.ROUTE_KEY_HEADER, abi.ROUTE_KEY_BYTES, abi.ROUTE_KEY_PARTITION, abi.ROUTE_DROP)


# ------------------------------------------------------------------ refusals
def test_refusals():
    bad, good = RU.malformed_specs()
    L = codec.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced
    for name, (src, spec) in bad.items():
        assert R.refused(spec, src), name
        rc, _ = _twin(src, 3, spec)
        assert rc == BAD, name
    for name, (src, spec) in good.items():
        assert not R.refused(spec, src), name
        rc, part = _twin(src, 3, spec)
        assert rc == 0 and np.array_equal(part, R.partitions_of(spec, src, 3)), name
    src, spec = good["by id"]
    s, q, part = U.src_struct(src, 3, _ptr), RU.abi_spec(spec, _ptr), np.zeros(4, np.uint32)
    assert L.iggy_route_partitions_host(None, 3, ctypes.byref(q), part.ctypes.data) == BAD
    assert L.iggy_route_partitions_host(ctypes.byref(s), 3, None, part.ctypes.data) == BAD
    assert L.iggy_route_partitions_host(ctypes.byref(s), 3, ctypes.byref(q), None) == BAD
    assert L.iggy_route_partitions_host(ctypes.byref(s), 4, ctypes.byref(q), part.ctypes.data) == BAD  # above cap_messages
    assert L.iggy_route_partitions_host(ctypes.byref(s), 3, ctypes.byref(q), part.ctypes.data) == 0
    # the device entry: no context exists without a device, and a null context is refused
    # with a null stream (the GPU suite repeats every refusal with a live one)
    call = L.iggy_codec_route_messages_device
    assert call(None, ctypes.byref(s), p, ctypes.byref(q), None, p, None, None, None, None, p, None) == BAD


# ------------------------------------------------------------------ the host twin
def _mask(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.7).astype(np.uint8)


@pytest.mark.parametrize("partitions", [1, 2, 3, 255, 256])
def test_by_id(partitions):
    src = U.make_source(np.arange(500) % 9, seed=3)
    for mask in (None, _mask(500, 4)):
        spec = R.Spec(partitions, R.KEY_ID, mask=mask)
        rc, part = _twin(src, 500, spec)
        want = R.partitions_of(spec, src, 500)
        assert rc == 0 and np.array_equal(part, want)
        live = want[want != R.DROP]
        assert live.size and live.max() < partitions
        if mask is not None:
            assert np.array_equal(want == R.DROP, mask == 0)
    ids = src["ids"]
    key = int(ids[0]).to_bytes(8, "little") + int(ids[1]).to_bytes(8, "little")
    assert int(part[0]) in (R.xxh32(key) % partitions, R.DROP)


@pytest.mark.parametrize("length", [1, 3, 4, 8, 15, 16, 17, 31, 32, 33, 255])
def test_by_bytes(length):
    rng = np.random.default_rng(length)
    for stride in (length, length + 5):
        keys = rng.integers(0, 256, size=(64, stride), dtype=np.uint8)
        spec = R.Spec(7, R.KEY_BYTES, key_length=length, key_stride=stride, keys=keys)
        rc, part = _twin(U.make_source(np.zeros(64, np.uint32)), 64, spec)
        assert rc == 0 and np.array_equal(part, R.partitions_of(spec, {}, 64))
        assert int(part[5]) == R.xxh32(bytes(keys[5, :length])) % 7
    # messages_key_u32 / _u64: the little-endian bytes of the value
    if length in (4, 8):
        v = 0x1234567890ABCDEF % (1 << (8 * length))
        keys = np.frombuffer(v.to_bytes(length, "little"), np.uint8).reshape(1, length).copy()
        spec = R.Spec(10, R.KEY_BYTES, key_length=length, key_stride=length, keys=keys)
        rc, part = _twin(U.make_source([0]), 1, spec)
        assert rc == 0 and int(part[0]) == R.xxh32(v.to_bytes(length, "little")) % 10


def test_by_header_absent_to_a_partition_and_to_drop():
    rng = np.random.default_rng(8)
    keys = [None if i % 6 == 0 else bytes(rng.integers(0, 256, size=[1, 16, 17, 255, 4][i % 5], dtype=np.uint8))
            for i in range(200)]
    src, col = RU.header_source(keys)
    for absent in (R.DROP, 0, 4):
        for mask in (None, _mask(200, 9)):
            spec = R.Spec(5, R.KEY_HEADER, absent, column=col, mask=mask)
            rc, part = _twin(src, 200, spec)
            want = R.partitions_of(spec, src, 200)
            assert rc == 0 and np.array_equal(part, want)
            if mask is None:
                assert (want[::6] == absent).all() and (want[1::6] != R.DROP).all()
    assert int(want[1]) in (R.xxh32(keys[1]) % 5, R.DROP)
    # a column entry that does not lie inside its message's header bytes counts as absent
    col2 = {k: v.copy() for k, v in col.items()}
    col2["value_pos"][1] += 1
    spec = R.Spec(5, R.KEY_HEADER, 3, column=col2)
    rc, part = _twin(src, 200, spec)
    assert rc == 0 and int(part[1]) == 3 and np.array_equal(part, R.partitions_of(spec, src, 200))


def test_by_partition_ids():
    ids = np.array([0, 1, 2, 3, 4, 5, 2**32 - 1, 2**31, 255, 256, 2, 2], dtype=np.uint32)
    src = U.make_source(np.zeros(ids.size, np.uint32))
    for partitions in (1, 3, 256):
        for mask in (None, _mask(ids.size, 10)):
            spec = R.Spec(partitions, R.KEY_PARTITION, partition_ids=ids, mask=mask)
            rc, part = _twin(src, ids.size, spec)
            want = R.partitions_of(spec, src, ids.size)
            assert rc == 0 and np.array_equal(part, want)
            if mask is None:
                assert np.array_equal(want, np.where(ids < partitions, ids, R.DROP))


def test_restatement_orders_by_partition_then_source():
    src = U.make_source(np.arange(300) % 11, np.arange(300) % 3, seed=12)
    x = R.route(R.Spec(4, R.KEY_ID, mask=_mask(300, 13)), src, 300)
    p = x["partition_of"][x["source_index"].astype(np.int64)]
    assert (np.diff(p.astype(np.int64)) >= 0).all() and x["count"] + x["dropped"] == 300
    for a, b in zip(x["partition_first"][:-1], x["partition_first"][1:]):
        assert (np.diff(x["source_index"][int(a):int(b)].astype(np.int64)) > 0).all()
    assert x["partition_first"][-1] == x["count"] and x["partition_payload_first"][-1] == x["payload_bytes"]
