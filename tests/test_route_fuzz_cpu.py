"""Stand-alone host sanitizer run of the route's host twin: iggy_amd/csrc/route.cpp ALONE
(with route_key.hpp and xxh32.hpp, the hash and the partition rule the device kernel
shares), built with g++ -fsanitize=address,undefined into tests/fuzz/route_host_fuzz.cpp
(its own main), fed seeded sources and specs on stdin. Every array lives in a heap block
that ends at the array's last byte; key arrays and header blobs start at every offset
0..15 of a block, so a key's tail read past its end is an AddressSanitizer report. Any
sanitizer report aborts the harness and fails the test; its printed partitions (and
refusals) are also compared with the restatement (tests/route_ref.py). Nothing is loaded
into Python. No GPU."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import route_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iggy_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "fuzz", "route_host_fuzz.cpp"), os.path.join(CSRC, "route.cpp")]
DEPS = SRC + [os.path.join(CSRC, "route_key.hpp"), os.path.join(CSRC, "xxh32.hpp"),
              os.path.join(ROOT, "include", "iggy_codec.h")]
OUT = os.path.join(ROOT, "build", "route_host_fuzz_asan")
SEED = 7411
LENGTHS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 19, 31, 32, 33, 47, 64, 100, 254, 255]


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


def _arr(name, a, off=0, n=1):
    """(an empty array still gets a block, of one zero byte, unless it is left out)"""
    return f"A {name} {off} {_hex(a) if n and len(_hex(a)) > 1 else '00'}"


def _case(rng, shift):
    """-> (lines defining a source, n, src, keys, key_length, stride, partition_ids, column, mask)."""
    n = rng.choice([0, 1, 2, 7, 33])
    lines = [f"N {n}"]
    src = {}
    if rng.random() < 0.9:
        src["ids"] = np.array([rng.getrandbits(64) for _ in range(2 * n)], dtype=np.uint64)
        lines.append(_arr("ids", src["ids"], 0, n))
    # header blobs: [filler | key]; the key ends its message's bytes, so the last one ends the block
    hk = [None if rng.random() < 0.2 else bytes(rng.getrandbits(8) for _ in range(rng.choice(LENGTHS)))
          for _ in range(n)]
    fill = [rng.randrange(0, 6) if k is not None else rng.choice([0, 0, 3]) for k in hk]
    blobs = [bytes(f) + (k or b"") for f, k in zip(fill, hk)]
    if rng.random() < 0.9:
        src["user_headers_starts"] = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
        lines.append(_arr("user_headers_starts", src["user_headers_starts"]))
    if rng.random() < 0.9:
        src["user_headers"] = np.frombuffer(b"".join(blobs), np.uint8).copy()
        lines.append(_arr("user_headers", src["user_headers"], shift, len(src["user_headers"])))
    col = {}
    wild = rng.random() < 0.15  # now and then a column of other messages
    for name, vals, dt in (("value_kinds", [0 if k is None else rng.randint(1, 15) for k in hk], np.uint8),
                           ("value_lengths", [0 if k is None else len(k) for k in hk], np.uint8),
                           ("value_pos", [f + (rng.choice([0, 1, 300]) if wild else 0) for f in fill], np.uint32)):
        if rng.random() < 0.95:
            col[name] = np.array(vals, dtype=dt)
            lines.append(_arr(name, col[name], 0, n))
    klen = rng.choice(LENGTHS)
    stride = klen + rng.choice([0, 0, 1, 5])
    keys = None
    if rng.random() < 0.9:  # (the array ends with its last key: no stride padding after it)
        keys = np.array([rng.getrandbits(8) for _ in range(max(n - 1, 0) * stride + (klen if n else 0))], dtype=np.uint8)
        lines.append(_arr("keys", keys, (shift * 7 + 3) % 16, keys.size))
    pids = None
    if rng.random() < 0.9:
        pids = np.array([rng.choice([0, 1, 2, 5, 255, 256, 2**32 - 1, rng.randrange(0, 300)]) for _ in range(n)],
                        dtype=np.uint32)
        lines.append(_arr("partition_ids", pids, 0, n))
    mask = None
    if rng.random() < 0.4:
        mask = np.array([rng.choice([0, 1, 255]) for _ in range(n)], dtype=np.uint8)
        lines.append(_arr("mask", mask, 0, n))
    return lines, n, src, keys, klen, stride, pids, col, mask


def _sample(seed=SEED):
    rng = random.Random(seed)
    lines, expect = [], []
    for c in range(500):
        defs, n, src, keys, klen, stride, pids, col, mask = _case(rng, c % 16)
        lines += defs
        for _ in range(4):
            wild = rng.random() < 0.08
            partitions = rng.choice([0, 257, 2**32 - 1]) if wild else rng.choice([1, 2, 3, 7, 255, 256])
            source = rng.randint(0, 5) if rng.random() < 0.05 else rng.randint(1, 4)
            absent = rng.choice([R.DROP, R.DROP, 0, partitions - 1 if partitions else 0, partitions, 1000])
            kl, ks = (rng.choice([0, 256]), stride) if rng.random() < 0.03 else (klen, stride)
            if rng.random() < 0.03:
                ks = max(kl - 1, 0)
            # (a key length other than the case's own is one the entry refuses: 0, 256, or above the stride)
            spec = R.Spec(partitions, source, absent, kl, ks, keys, pids, col, mask)
            lines.append(f"Q {partitions} {source} {absent} {kl} {ks}")
            if R.refused(spec, src):
                expect.append((R.ERR_INVALID_ARGUMENT, None))
            else:
                expect.append((0, R.partitions_of(spec, src, n)))
    return lines, expect


def _census(expect):
    refused = sum(1 for rc, _ in expect if rc)
    parts = np.concatenate([p for rc, p in expect if not rc and p.size] + [np.zeros(0, np.uint32)])
    return refused, int((parts == R.DROP).sum()), set(parts[parts != R.DROP].tolist())


def test_the_restatement_alone_decides_every_way():
    """The sample holds refusals, drops and at least three distinct partitions, by the
    restatement alone (no library, no harness)."""
    refused, drops, distinct = _census(_sample()[1])
    assert refused > 50 and drops > 500 and len(distinct) >= 3, (refused, drops, len(distinct))


def test_route_fuzz(harness):
    lines, expect = _sample()
    out = _run(harness, lines)
    assert len(out) == len(expect)
    for line, (rc, part) in zip(out, expect):
        got = line.split()
        assert int(got[0]) == rc, line
        if rc == 0:
            assert got[1:] == ([str(int(p)) for p in part] or ["-"]), line
    refused, drops, distinct = _census(expect)
    assert refused > 50 and drops > 500 and len(distinct) >= 3


def test_hash_tails_at_every_offset(harness):
    """One key alone in a block, at every offset 0..15 of the block's start and ending at its
    last byte, for every length 0..48 and the long ones."""
    rng = random.Random(SEED + 1)
    lines, want = [], []
    for n in list(range(49)) + [63, 64, 65, 127, 128, 254, 255]:
        for off in range(16):
            data = bytes(rng.getrandbits(8) for _ in range(n))
            lines.append(f"H {off} {_hex(data)}")
            want.append(R.xxh32(data))
    out = _run(harness, lines)
    assert [int(x) for x in out] == want
