"""Stand-alone host sanitizer run of the user-header host twin: iggy_amd/csrc/
user_headers.cpp ALONE, built with g++ -fsanitize=address,undefined into
tests/fuzz/user_headers_host_fuzz.cpp (its own main), fed seeded random, mutated and
truncated buffers on stdin. The harness checks that every out-parameter lies inside the
buffer; any sanitizer report aborts it and fails the test; its printed verdicts are also
compared with the restatement (tests/user_headers_ref.py). Nothing is loaded into Python.
No GPU."""
import os
import random
import shutil
import subprocess

import pytest

import user_headers_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "fuzz", "user_headers_host_fuzz.cpp"),
       os.path.join(ROOT, "iggy_amd", "csrc", "user_headers.cpp")]
DEPS = SRC + [os.path.join(ROOT, "iggy_amd", "csrc", "user_headers_walk.hpp"),
              os.path.join(ROOT, "include", "iggy_codec.h")]
OUT = os.path.join(ROOT, "build", "user_headers_host_fuzz_asan")
KEYS = [(2, b"route"), (2, b"rout"), (1, b"route"), (6, b"\x07\x00\x00\x00"), (2, b"k" * 255)]


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


def _hex(b: bytes) -> str:
    return b.hex() if b else "-"


def _buffers(rng, n):
    out = [b"", b"\x01", b"\x00", b"\x01\xff\xff\xff\xff", b"\x02\x03\x00\x00\x00ab"]
    for _ in range(n):
        r = rng.random()
        if r < 0.25:
            buf = rng.randbytes(rng.randint(0, 40))
        else:
            parts = []
            for _ in range(rng.randint(1, 10)):
                kk, key = rng.choice(KEYS)
                vk = rng.randint(1, 15)
                size = R.EXPECTED_SIZE[vk]
                parts.append(R.pair(kk, key, vk, rng.randbytes(size if size is not None else rng.choice([1, 16, 17, 255]))))
            buf = b"".join(parts)
            if r < 0.6:  # one byte changed (kinds and lengths among them)
                i = rng.randrange(len(buf))
                buf = buf[:i] + bytes([rng.choice([0, 1, 16, 255, rng.randrange(256)])]) + buf[i + 1:]
            if rng.random() < 0.5:  # every kind of truncation
                buf = buf[:rng.randint(0, len(buf))]
        out.append(buf)
    return out


def test_validate_fuzz(harness):
    rng = random.Random(2201)
    bufs = _buffers(rng, 4000)
    out = _run(harness, ["V " + _hex(b) for b in bufs])
    assert len(out) == len(bufs)
    for b, line in zip(bufs, out):
        f = [int(x) for x in line.split()[1:]]
        status, pairs, _ = R.decode(b)
        assert (tuple(f[:4]), f[4]) == (status, pairs), b.hex()


def test_get_fuzz(harness):
    rng = random.Random(2202)
    bufs = _buffers(rng, 3000)
    keys = [rng.choice(KEYS) for _ in bufs]
    out = _run(harness, [f"G {k[0]} {_hex(k[1])} {_hex(b)}" for k, b in zip(keys, bufs)])
    assert len(out) == len(bufs)
    found = 0
    for b, k, line in zip(bufs, keys, out):
        f = [int(x) for x in line.split()[1:]]
        want = R.decode(b)
        vk, vp, vl, _ = R.lookup(want, k)
        assert (tuple(f[:4]), tuple(f[4:])) == (want[0], (vk, vp, vl)), (b.hex(), k)
        found += vk != 0
    assert found > 200  # the lookups are not all misses
