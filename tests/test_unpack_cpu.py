"""The consumer unpack's C ABI without a GPU: the library exports the entry point, and
the three ctypes mirrors agree with include/iggy_codec.h field by field (the gcc
offsetof probe of tests/test_abi_layout_cpu.py, for the three new typedefs)."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import pytest

from iggy_amd import abi, codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "iggy_codec.h")


def _pairs():
    return {
        abi.UnpackedMessages: "iggy_unpacked_messages",
        abi.UnpackCursor: "iggy_unpack_cursor",
        abi.UnpackResult: "iggy_unpack_result",
    }


def test_library_exports_the_unpack_entry():
    assert "iggy_codec_unpack_batch_device" in codec.exported_symbols()
    assert hasattr(codec.lib(), "iggy_codec_unpack_batch_device")


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


@pytest.mark.parametrize("name", ["UnpackedMessages", "UnpackCursor", "UnpackResult"])
def test_mirror_matches_header(name, c_layout):
    cls = getattr(abi, name)
    cname = _pairs()[cls]
    assert ctypes.sizeof(cls) == c_layout[(cname, "size")], cname
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == c_layout[(cname, f)], (cname, f)
    assert ctypes.sizeof(abi.UnpackedMessages) == 112 and ctypes.sizeof(abi.UnpackCursor) == 32
    assert ctypes.sizeof(abi.UnpackResult) == 80
