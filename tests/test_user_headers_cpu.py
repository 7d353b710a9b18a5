"""User-header validation and key lookup without a GPU: the plain-Python restatement
(tests/user_headers_ref.py) reproduces the reference's own unit-test vectors
(tests/golden/user_headers_vectors.json), the host twin (iggy_user_headers_validate / _get,
iggy_amd/csrc/user_headers.cpp) equals the restatement on them and on 5 000 seeded random
or mutated buffers, the library exports the four entry points, the ctypes mirrors agree
with include/iggy_codec.h (the gcc offsetof probe of tests/test_unpack_cpu.py), and the
device entry points refuse malformed requests synchronously, with no device."""
import ctypes
import json
import os
import random
import shutil
import subprocess
import tempfile

import pytest

import user_headers_ref as R
from iggy_amd import abi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iggy_codec.h")
VECTORS = os.path.join(ROOT, "tests", "golden", "user_headers_vectors.json")


def _vectors():
    with open(VECTORS) as f:
        return json.load(f)["vectors"]


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("v", _vectors(), ids=lambda v: v["name"])
def test_restatement_reproduces_the_reference_vectors(v):
    buf = bytes.fromhex(v["input"])
    sstatus, tlvs = R.validate(buf)
    status, pairs, headers = R.decode(buf)
    if v["structural_pairs"] is not None:
        assert sstatus == R.STATUS_OK and len(tlvs) // 2 == v["structural_pairs"]
    else:
        assert sstatus != R.STATUS_OK and status == sstatus
    if v["outcome"] == "ok":
        assert status == R.STATUS_OK
    elif v["outcome"] == "validation":
        assert status[0] == R.ERR_VALIDATION
    elif v["outcome"] == "domain_error":
        assert sstatus == R.STATUS_OK and status[0] in (R.ERR_INVALID_HEADER_KEY, R.ERR_INVALID_HEADER_VALUE,
                                                         R.ERR_INVALID_HEADER_KIND)
    else:
        assert status[0] != R.OK
    assert list(status) == v["status"] and pairs == v["pairs"]
    want = {}
    for kk, key, vk, val in v["entries"]:
        want[(kk, bytes.fromhex(key))] = (vk, bytes.fromhex(val))
    assert {k: (x[0], x[3]) for k, x in headers.items()} == want
    for k, (vk, vp, vl, vb) in headers.items():
        assert buf[vp:vp + vl] == vb


# ------------------------------------------------------------------ the host twin
def _twin_validate(L, buf: bytes):
    st, pairs = abi.HeaderStatus(), ctypes.c_uint32(0xDEAD)
    rc = L.iggy_user_headers_validate(buf, len(buf), ctypes.byref(pairs), ctypes.byref(st))
    assert rc == st.kind
    return st.astuple(), pairs.value


def _twin_get(L, buf: bytes, key):
    st = abi.HeaderStatus()
    vk, vl, vp = ctypes.c_uint8(0xEE), ctypes.c_uint8(0xEE), ctypes.c_uint32(0xDEAD)
    k = abi.HeaderKey.make(*key)
    rc = L.iggy_user_headers_get(buf, len(buf), ctypes.byref(k), ctypes.byref(vk), ctypes.byref(vp),
                                 ctypes.byref(vl), ctypes.byref(st))
    assert rc == st.kind
    return st.astuple(), (vk.value, vp.value, vl.value)


def _agree(L, buf: bytes, keys):
    want = R.decode(buf)
    assert _twin_validate(L, buf) == (want[0], want[1]), buf.hex()
    for key in keys:
        st, got = _twin_get(L, buf, key)
        assert st == want[0] and got == R.lookup(want, key)[:3], (buf.hex(), key)


def test_host_twin_equals_the_restatement_on_the_vectors():
    L = codec.lib()
    for v in _vectors():
        buf = bytes.fromhex(v["input"])
        keys = [(kk, bytes.fromhex(k)) for kk, k, _, _ in v["entries"]] + [(2, b"absent")]
        _agree(L, buf, keys)


POOL = [(2, b"route"), (2, b"rout"), (1, b"route"), (6, b"\x01\x00\x00\x00"), (7, bytes(8)), (2, b"x" * 200),
        (3, b"\x01"), (13, bytes(range(16)))]


def random_value(rng):
    kind = rng.randint(1, 15)
    size = R.EXPECTED_SIZE[kind]
    return kind, rng.randbytes(size if size is not None else rng.choice([1, 2, 15, 16, 17, 40, 255]))


def random_headers(rng) -> bytes:
    """valid | valid but mutated in one byte | random bytes (also used by the GPU seeded mix)"""
    r = rng.random()
    if r < 0.2:
        return rng.randbytes(rng.choice([0, 1, 4, 5, 6, 11, 30]))
    buf = b"".join(R.pair(*rng.choice(POOL), *random_value(rng)) for _ in range(rng.randint(1, 12)))
    if r < 0.6:
        i = rng.randrange(len(buf))
        buf = buf[:i] + bytes([rng.choice([0, 1, 2, 16, 255, rng.randrange(256)])]) + buf[i + 1:]
        if rng.random() < 0.3:
            buf = buf[:rng.randint(0, len(buf))]
    return buf


def test_host_twin_equals_the_restatement_on_random_buffers():
    L = codec.lib()
    rng = random.Random(1107)
    kinds = set()
    for _ in range(5000):
        buf = random_headers(rng)
        kinds.add(R.decode(buf)[0][:2] if R.decode(buf)[0][0] != R.ERR_INVALID_HEADER_KIND else (29, 0))
        _agree(L, buf, rng.sample(POOL, 3))
    # every verdict class is in the sample
    assert {(0, 0), (1, 0), (2, 11), (2, 12), (2, 13), (27, 0), (28, 0), (29, 0)} <= kinds


def test_host_twin_refuses_a_malformed_key():
    L = codec.lib()
    buf = R.pair(2, b"k", 2, b"v")
    bad = abi.ERR_INVALID_ARGUMENT
    assert L.iggy_user_headers_get(buf, len(buf), None, None, None, None, None) == bad
    for key in ((0, b"k"), (16, b"k"), (2, b""), (6, b"abc")):
        k = abi.HeaderKey.make(*key)
        assert L.iggy_user_headers_get(buf, len(buf), ctypes.byref(k), None, None, None, None) == bad
    assert L.iggy_user_headers_validate(None, 0, None, None) == 0  # an empty buffer is valid


# ------------------------------------------------------------------ exports, mirrors
NAMES = ("iggy_codec_user_headers_device", "iggy_codec_user_headers_arrays_device",
         "iggy_user_headers_validate", "iggy_user_headers_get")


def test_library_exports_the_entry_points():
    for name in NAMES:
        assert name in codec.exported_symbols()
        assert hasattr(codec.lib(), name)


def test_error_strings():
    L = codec.lib()
    L.iggy_codec_error_string.restype = ctypes.c_char_p
    texts = {L.iggy_codec_error_string(k, r) for k, r in ((27, 0), (28, 0), (29, 0), (2, 11), (2, 12), (2, 13))}
    assert len(texts) == 6 and b"unknown" not in texts and b"validation failed" not in texts


def _pairs():
    return {
        abi.HeaderKey: "iggy_header_key",
        abi.HeaderStatus: "iggy_header_status",
        abi.HeaderColumn: "iggy_header_column",
        abi.HeaderColumns: "iggy_header_columns",
        abi.HeaderColumnsResult: "iggy_header_columns_result",
    }


@pytest.fixture(scope="module")
def c_layout():
    cc = shutil.which("gcc")
    if not cc:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for cls, cname in _pairs().items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    for name in ("IGGY_ERR_INVALID_HEADER_KEY", "IGGY_ERR_INVALID_HEADER_VALUE", "IGGY_ERR_INVALID_HEADER_KIND",
                 "IGGY_V_HEADER_KIND_ZERO", "IGGY_V_HEADER_FIELD_LENGTH", "IGGY_V_HEADER_ODD_ENTRIES"):
        lines.append(f'printf("enum {name} %d\\n", (int){name});')
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


@pytest.mark.parametrize("name", ["HeaderKey", "HeaderStatus", "HeaderColumn", "HeaderColumns",
                                  "HeaderColumnsResult"])
def test_mirror_matches_header(name, c_layout):
    cls = getattr(abi, name)
    cname = _pairs()[cls]
    assert ctypes.sizeof(cls) == c_layout[(cname, "size")], cname
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == c_layout[(cname, f)], (cname, f)
    assert ctypes.sizeof(abi.HeaderKey) % 8 == 0 and ctypes.sizeof(abi.HeaderStatus) == 16


def test_enum_values(c_layout):
    assert [c_layout[("enum", n)] for n in ("IGGY_ERR_INVALID_HEADER_KEY", "IGGY_ERR_INVALID_HEADER_VALUE",
                                            "IGGY_ERR_INVALID_HEADER_KIND")] == [27, 28, 29]
    assert [c_layout[("enum", n)] for n in ("IGGY_V_HEADER_KIND_ZERO", "IGGY_V_HEADER_FIELD_LENGTH",
                                            "IGGY_V_HEADER_ODD_ENTRIES")] == [11, 12, 13]
    assert (abi.ERR_INVALID_HEADER_KEY, abi.ERR_INVALID_HEADER_VALUE, abi.ERR_INVALID_HEADER_KIND) == (27, 28, 29)
    assert (abi.V_HEADER_KIND_ZERO, abi.V_HEADER_FIELD_LENGTH, abi.V_HEADER_ODD_ENTRIES) == (11, 12, 13)
    assert (R.ERR_INVALID_HEADER_KEY, R.V_HEADER_KIND_ZERO) == (27, 11)


# ------------------------------------------------------------------ synchronous refusals
def _request(keys):
    q = abi.HeaderColumns()
    q.cap_messages, q.nkeys = 4, len(keys)
    for k, key in enumerate(keys[:16]):
        q.keys[k] = abi.HeaderKey.make(*key)
    return q


def malformed_requests():
    """name -> request that the entry points refuse whatever the other arguments are"""
    return {
        "17 keys": _request([(2, b"k")] * 17),
        "length-0 key": _request([(2, b"ok"), (2, b"")]),
        "Int32 key of 3 bytes": _request([(6, b"abc")]),
        "kind 0": _request([(0, b"k")]),
        "kind 16": _request([(16, b"k")]),
        "1025 key bytes": _request([(2, b"a" * 255)] * 4 + [(2, b"b" * 5)]),
    }


def test_synchronous_refusals_without_a_device():
    """No context exists without a device, and a null context is refused: every call here
    returns before anything touches one (the GPU suite repeats the malformed requests with
    a live context, where 1024 key bytes are accepted)."""
    L = codec.lib()
    bad = abi.ERR_INVALID_ARGUMENT
    ok = _request([(2, b"k")])
    p = ctypes.c_void_p(4096)  # never dereferenced
    assert L.iggy_codec_user_headers_device(None, p, 512, p, p, ctypes.byref(ok), p, None) == bad
    assert L.iggy_codec_user_headers_arrays_device(None, p, p, p, 4, ctypes.byref(ok), p, None) == bad
    for name, q in malformed_requests().items():
        assert L.iggy_codec_user_headers_device(None, p, 512, p, p, ctypes.byref(q), p, None) == bad, name
        assert L.iggy_codec_user_headers_arrays_device(None, p, p, p, 4, ctypes.byref(q), p, None) == bad, name
