"""The select's C ABI and clause semantics without a GPU: the exports, the ctypes mirrors
against include/iggy_codec.h (the gcc offsetof probe of tests/test_unpack_cpu.py), the
synchronous refusals, and the host twin (iggy_select_mask_host, select.cpp, which shares
select_clause.hpp with the device kernel) against the plain-Python restatement
(tests/select_ref.py): every source, op and kind at its boundary values, absent keys and
kind mismatches under every op, and a seeded mix of 5 000 messages."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import select_ref as R
import select_util as U
from iggy_amd import abi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iggy_codec.h")
BAD = abi.ERR_INVALID_ARGUMENT


def _ptr(a):
    return a.ctypes.data


def _twin(src, count, clauses, mask=None, cap=None):
    spec = U.abi_spec(clauses, _ptr, mask)
    return codec.select_mask_host(U.src_struct(src, count if cap is None else cap, _ptr), count, spec)


# ------------------------------------------------------------------ exports, mirrors
def test_library_exports_the_entry_points():
    for name in ("iggy_codec_select_messages_device", "iggy_select_mask_host"):
        assert name in codec.exported_symbols()
        assert hasattr(codec.lib(), name)


def _pairs():
    return {abi.SelectClause: "iggy_select_clause", abi.SelectSpec: "iggy_select_spec",
            abi.SelectResult: "iggy_select_result"}


CONSTANTS = {"IGGY_SELECT_MAX_CLAUSES": abi.SELECT_MAX_CLAUSES, "IGGY_SEL_OFFSET": abi.SEL_OFFSET,
             "IGGY_SEL_TIMESTAMP": abi.SEL_TIMESTAMP, "IGGY_SEL_ORIGIN_TIMESTAMP": abi.SEL_ORIGIN_TIMESTAMP,
             "IGGY_SEL_PAYLOAD_LENGTH": abi.SEL_PAYLOAD_LENGTH,
             "IGGY_SEL_USER_HEADERS_LENGTH": abi.SEL_USER_HEADERS_LENGTH, "IGGY_SEL_ID": abi.SEL_ID,
             "IGGY_SEL_HEADER": abi.SEL_HEADER, "IGGY_SEL_HEADER_STATUS": abi.SEL_HEADER_STATUS,
             "IGGY_OP_EQ": abi.OP_EQ, "IGGY_OP_NE": abi.OP_NE, "IGGY_OP_LT": abi.OP_LT, "IGGY_OP_LE": abi.OP_LE,
             "IGGY_OP_GT": abi.OP_GT, "IGGY_OP_GE": abi.OP_GE, "IGGY_OP_PRESENT": abi.OP_PRESENT,
             "IGGY_OP_ABSENT": abi.OP_ABSENT}


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


@pytest.mark.parametrize("name", ["SelectClause", "SelectSpec", "SelectResult"])
def test_mirror_matches_header(name, c_layout):
    cls = getattr(abi, name)
    cname = _pairs()[cls]
    assert ctypes.sizeof(cls) == c_layout[(cname, "size")], cname
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == c_layout[(cname, f)], (cname, f)


def test_constants_match_header(c_layout):
    for name, value in CONSTANTS.items():
        assert c_layout[("const", name)] == value, name
    assert (R.SEL_HEADER_STATUS, R.OP_ABSENT, R.K_FLOAT64) == (abi.SEL_HEADER_STATUS, abi.OP_ABSENT, abi.KIND_FLOAT64)


# ------------------------------------------------------------------ refusals
def test_refusals():
    bad, good = U.malformed_specs()
    L = codec.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced
    for name, (src, clauses) in bad.items():
        assert R.refused(clauses, src), name
        rc, _ = _twin(src, 3, clauses)
        assert rc == BAD, name
        # (no context exists without a device, and a null context is refused: the GPU suite
        # repeats the malformed specs with a live one)
        spec, s = U.abi_spec(clauses, _ptr), U.src_struct(src, 3, _ptr)
        assert L.iggy_codec_select_messages_device(None, ctypes.byref(s), p, ctypes.byref(spec), ctypes.byref(s),
                                                   None, None, p, None) == BAD, name
    for name, (src, clauses) in good.items():
        assert not R.refused(clauses, src), name
        rc, keep = _twin(src, 3, clauses)
        assert rc == 0 and np.array_equal(keep.astype(bool), R.keep_mask(src, 3, clauses)), name
    src = U.make_source([1, 2, 3])
    s, spec, keep = U.src_struct(src, 3, _ptr), U.abi_spec([], _ptr), np.zeros(4, np.uint8)
    assert L.iggy_select_mask_host(None, 3, ctypes.byref(spec), keep.ctypes.data) == BAD
    assert L.iggy_select_mask_host(ctypes.byref(s), 3, None, keep.ctypes.data) == BAD
    assert L.iggy_select_mask_host(ctypes.byref(s), 3, ctypes.byref(spec), None) == BAD
    assert L.iggy_select_mask_host(ctypes.byref(s), 4, ctypes.byref(spec), keep.ctypes.data) == BAD  # above cap_messages
    assert L.iggy_select_mask_host(ctypes.byref(s), 3, ctypes.byref(spec), keep.ctypes.data) == 0


# ------------------------------------------------------------------ the boundary table
def test_plain_sources_at_their_boundaries():
    src, clauses = U.plain_cases()
    n = src["offsets"].size
    seen = set()
    for c in clauses:
        want = R.keep_mask(src, n, [c])
        rc, keep = _twin(src, n, [c])
        assert rc == 0 and np.array_equal(keep.astype(bool), want), c
        seen |= {(c.source, c.op, bool(v)) for v in want}
    for s in (*R.U64_SOURCES, *R.U32_SOURCES, R.SEL_ID):
        for op in R.COMPARE_OPS:
            assert (s, op, True) in seen and (s, op, False) in seen, (s, op)


@pytest.mark.parametrize("group", ["signed", "unsigned", "float32", "float64", "bool", "text"])
def test_header_kinds_at_their_boundaries(group):
    src = {}
    both = set()
    for g, col, clauses in U.header_cases():
        if g != group:
            continue
        n = col["value_kinds"].size
        for c in clauses:
            want = R.keep_mask(src, n, [c])
            rc, keep = _twin(src, n, [c])
            assert rc == 0 and np.array_equal(keep.astype(bool), want), (c.kind, c.op, c.operand.hex(), keep, want)
            both |= {(c.kind, c.op, bool(v)) for v in want}
            if c.op in R.COMPARE_OPS:  # absent keys and kind mismatches (the last two rows): false under every op
                assert not want[-2:].any() and not keep[-2:].any()
    assert both
    for kind, op, _ in list(both):
        assert (kind, op, True) in both and (kind, op, False) in both, (kind, op)


def test_the_named_boundaries():
    """The pairs the contract names, spelled out (the table above holds them too)."""
    def one(kind, stored, op, operand, length=None):
        col = U.column([(kind, len(stored) if length is None else length, stored)])
        c = R.clause(R.SEL_HEADER, op, operand, kind, col)
        rc, keep = _twin({}, 1, [c])
        assert rc == 0 and bool(keep[0]) == R.clause_true(c, {}, 0)
        return bool(keep[0])
    i = U._i
    assert one(R.K_INT8, i(-128, 1, True), R.OP_LT, i(127, 1, True))
    assert not one(R.K_INT8, i(127, 1, True), R.OP_LT, i(-128, 1, True))
    assert one(R.K_UINT64, i(2**63 - 1, 8, False), R.OP_LT, i(2**63, 8, False))
    assert one(R.K_INT64, i(2**63 - 1, 8, True), R.OP_GT, i(-2**63, 8, True))
    assert one(R.K_INT128, i(-1, 16, True), R.OP_LT, i(0, 16, True))
    assert one(R.K_UINT128, i(1 << 127, 16, False), R.OP_GT, i((1 << 127) - 1, 16, False))
    assert one(R.K_FLOAT32, U._f32(0x80000000), R.OP_EQ, U._f32(0))        # -0 == +0
    assert not one(R.K_FLOAT32, U._f32(0x80000000), R.OP_LT, U._f32(0))
    assert one(R.K_FLOAT32, U._f32(1), R.OP_GT, U._f32(0))                 # a denormal is above zero
    assert one(R.K_FLOAT64, U._f64(0x8000000000000001), R.OP_LT, U._f64(0x8000000000000000))
    assert one(R.K_FLOAT64, U._f64(0xFFF0000000000000), R.OP_LT, U._f64(0x7FF0000000000000))
    for nan in (0x7FC00000, 0xFFC00001):
        for op in R.COMPARE_OPS:
            assert one(R.K_FLOAT32, U._f32(nan), op, U._f32(nan)) == (op == R.OP_NE)
            assert one(R.K_FLOAT32, U._f32(0x3FC00000), op, U._f32(nan)) == (op == R.OP_NE)
    assert one(R.K_STRING, U.S16, R.OP_EQ, U.S16)
    assert not one(R.K_STRING, U.S16 + b"!", R.OP_EQ, U.S16, length=17)   # 17 stored, the first 16 match
    assert one(R.K_STRING, U.S16 + b"!", R.OP_NE, U.S16, length=17)
    assert not one(R.K_RAW, b"a\x00", R.OP_EQ, b"a")
    assert one(R.K_RAW, U.S15, R.OP_EQ, U.S15)


# ------------------------------------------------------------------ the seeded mix
def test_seeded_mix():
    src, specs = U.seeded_mix()
    n = src["offsets"].size
    assert n == 5000 and max(len(c) for c, _ in specs) == 8
    decided = set()
    kept = total = 0
    for clauses, mask in specs:
        want = R.keep_mask(src, n, clauses, mask)
        rc, keep = _twin(src, n, clauses, mask)
        assert rc == 0 and np.array_equal(keep.astype(bool), want)
        assert 0 < want.sum() < n  # no spec keeps everything or nothing
        kept, total = kept + int(want.sum()), total + n
        for c in clauses:
            alone = R.keep_mask(src, n, [c])
            decided |= {("op", c.op, bool(v)) for v in (alone.any(), alone.all())}
            decided |= {("source", c.source, bool(v)) for v in (alone.any(), alone.all())}
    # the restatement alone: between 20 % and 80 % kept, every op and source decides both ways
    assert 0.2 <= kept / total <= 0.8, kept / total
    for op in range(1, 9):
        assert ("op", op, True) in decided and ("op", op, False) in decided, op
    for s in range(1, 9):
        assert ("source", s, True) in decided and ("source", s, False) in decided, s
