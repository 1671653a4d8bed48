"""The head / body / tail split of a span of 4-byte entries for 16-byte stores
(emqx_amd/csrc/layout.h span_split, the staged CSR scatter's copy-out), on the CPU
(tests/c/test_span_split.cpp): every start offset within a 16-byte block and lengths 0..40 —
the parts add up, the vector region is 16-byte aligned and no store leaves the span.  Built
plainly and with the host sanitizers; the program has its own main and runs directly."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="no g++")
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_span_split(tmp_path, san):
    exe = tmp_path / "test_span_split"
    subprocess.run([GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *san,
                    "-I", os.path.join(ROOT, "emqx_amd/csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests/c/test_span_split.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
