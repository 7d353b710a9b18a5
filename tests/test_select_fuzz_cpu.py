"""Stand-alone host sanitizer run of the select's host twin: iggy_amd/csrc/select.cpp ALONE
(with select_clause.hpp, the clause evaluation the device kernel shares), built with
g++ -fsanitize=address,undefined into tests/fuzz/select_host_fuzz.cpp (its own main), fed
seeded sources and specs on stdin. Every array lives in a heap block of exactly its size;
any sanitizer report aborts the harness and fails the test; its printed verdicts (and
refusals) are also compared with the restatement (tests/select_ref.py). Nothing is loaded
into Python. No GPU."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "fuzz", "select_host_fuzz.cpp"),
       os.path.join(ROOT, "iggy_amd", "csrc", "select.cpp")]
DEPS = SRC + [os.path.join(ROOT, "iggy_amd", "csrc", "select_clause.hpp"),
              os.path.join(ROOT, "include", "iggy_codec.h")]
OUT = os.path.join(ROOT, "build", "select_host_fuzz_asan")
ARRAYS = ("offsets", "timestamps", "origin_timestamps", "payload_lengths", "user_headers_lengths", "ids")


def _build():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(s) for s in DEPS):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-Wall", "-o", OUT] + SRC
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return OUT


@pytest.fixture(scope="module")
def harness():
    return _build()


def _run(harness, lines):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([harness], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return p.stdout.splitlines()


def _hex(a) -> str:
    b = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
    return b.hex() if b else "-"


SPECIAL = [0, 1, 0x7F, 0x80, 0xFF, 2**15, 2**31 - 1, 2**31, 2**32 - 1, 2**63 - 1, 2**63, 2**64 - 1]


def _value(rng, kind):
    """Stored bytes of one value of `kind`, biased to its boundaries -> (length, bytes)."""
    if kind in (R.K_RAW, R.K_STRING):
        n = rng.choice([1, 2, 15, 16, 17, 40])
        return n, bytes(rng.choice(b"ab") for _ in range(n))
    size = R.KIND_SIZE[kind]
    if kind == R.K_FLOAT32:
        return 4, rng.choice([0, 0x80000000, 1, 0x80000001, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001,
                              0x3FC00000, 0xBFC00000]).to_bytes(4, "little")
    if kind == R.K_FLOAT64:
        return 8, rng.choice([0, 1 << 63, 1, (1 << 63) | 1, 0x7FF << 52, 0xFFF << 52, (0x7FF << 52) | 1,
                              0x3FF8 << 48, 0xBFF8 << 48]).to_bytes(8, "little")
    v = rng.choice([0, 1, (1 << (8 * size - 1)) - 1, 1 << (8 * size - 1), (1 << (8 * size)) - 1, rng.getrandbits(8 * size)])
    return size, v.to_bytes(size, "little")


def _case(rng):
    """-> (lines defining a source, the source dict, columns, statuses, mask)."""
    n = rng.choice([0, 1, 2, 7, 33])
    src = {}
    lines = [f"N {n}"]
    for name in ARRAYS:
        if rng.random() < 0.1:
            continue
        if name.endswith("_lengths"):
            a = np.array([rng.choice(SPECIAL) % 2**32 for _ in range(n)], dtype=np.uint32)
        else:
            a = np.array([rng.choice(SPECIAL) for _ in range(n * (2 if name == "ids" else 1))], dtype=np.uint64)
        src[name] = a
        lines.append(f"A {name} {_hex(a) if n else '00'}")
    cols, stats = [], []
    for k in range(3):
        kind = rng.randint(1, 15)
        col = {"value_kinds": np.zeros(n, np.uint8), "value_lengths": np.zeros(n, np.uint8),
               "values16": np.zeros((n, 16), np.uint8)}
        for i in range(n):
            r = rng.random()
            kk = 0 if r < 0.15 else rng.randint(1, 15) if r < 0.3 else kind
            if kk:
                ln, b = _value(rng, kk)
                col["value_kinds"][i], col["value_lengths"][i] = kk, ln
                col["values16"][i, :min(ln, 16)] = np.frombuffer(b[:16], np.uint8)
        col["kind"] = kind
        cols.append(col)
        lines.append(f"C {k} {_hex(col['value_kinds']) if n else '00'} {_hex(col['value_lengths']) if n else '00'} "
                     f"{_hex(col['values16']) if n else '00'}")
    st = np.zeros((n, 4), np.uint32)
    for i in range(n):
        st[i, 0] = rng.choice([0, 0, 0, 1, 2, 29])
    stats.append(st)
    lines.append(f"T 0 {_hex(st) if n else '00'}")
    mask = np.array([rng.choice([0, 1, 255]) for _ in range(n)], dtype=np.uint8)
    lines.append(f"M {_hex(mask) if n else '00'}")
    return lines, n, src, cols, stats, mask


def _clause(rng, cols, stats):
    r = rng.random()
    wild = rng.random() < 0.06  # now and then a malformed one
    if r < 0.4:
        source = rng.choice([R.SEL_OFFSET, R.SEL_TIMESTAMP, R.SEL_ORIGIN_TIMESTAMP, R.SEL_PAYLOAD_LENGTH,
                             R.SEL_USER_HEADERS_LENGTH, R.SEL_ID])
        op = rng.randint(0, 9) if wild else rng.choice(R.COMPARE_OPS)
        v = rng.choice(SPECIAL) | ((rng.choice(SPECIAL) << 64) if source == R.SEL_ID else 0)
        return R.clause(source, op, v.to_bytes(16, "little")), -1, -1
    if r < 0.5:
        return R.clause(R.SEL_HEADER_STATUS, rng.randint(0, 9), status=stats[0]), -1, 0
    k = rng.randrange(len(cols))
    col = cols[k]
    if r < 0.6:
        return R.clause(R.SEL_HEADER, rng.choice([R.OP_PRESENT, R.OP_ABSENT]), column=col), k, -1
    kind = rng.randint(0, 16) if wild else col["kind"]
    op = rng.randint(0, 9) if wild else rng.choice(R.COMPARE_OPS if kind > 3 else (R.OP_EQ, R.OP_NE))
    ln, b = _value(rng, kind if 1 <= kind <= 15 else 6)
    if ln > 16:
        ln, b = 16, b[:16]
    if wild and rng.random() < 0.5:
        ln = rng.choice([0, 3, 17])
    return R.clause(R.SEL_HEADER, op, (b + bytes(16))[:16], kind, col, length=ln), k, -1


def test_select_fuzz(harness):
    rng = random.Random(5207)
    lines, expect = [], []
    for _ in range(400):
        defs, n, src, cols, stats, mask = _case(rng)
        lines += defs
        for _ in range(6):
            picked = [_clause(rng, cols, stats) for _ in range(rng.choice([0, 1, 1, 2, 3, 8, 9]))]
            use_mask = rng.random() < 0.3
            q = [f"Q {int(use_mask)} {len(picked)}"]
            for c, ci, si in picked[:8]:
                q.append(f"{c.source} {c.op} {c.kind} {c.length} {_hex(c.operand)} {ci} {si}")
            lines.append(" ".join(q))
            cl = [c for c, _, _ in picked]
            if R.refused(cl, src):
                expect.append((R.ERR_INVALID_ARGUMENT, None))
            else:
                expect.append((0, R.keep_mask(src, n, cl, mask if use_mask else None)))
    out = _run(harness, lines)
    assert len(out) == len(expect)
    refused = kept = dropped = 0
    for line, (rc, keep) in zip(out, expect):
        got_rc, got = line.split()
        assert int(got_rc) == rc, line
        if rc:
            refused += 1
            continue
        want = "".join("01" if k else "00" for k in keep) or "-"
        assert got == want, line
        kept, dropped = kept + int(keep.sum()), dropped + int((~keep).sum())
    # the sample decides both ways and holds refusals too
    assert refused > 50 and kept > 1000 and dropped > 1000, (refused, kept, dropped)
