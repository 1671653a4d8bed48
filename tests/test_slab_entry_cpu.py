"""The fast-slab entry formats and the host-side format choice (emqx_amd/csrc/layout.h), on the
CPU (tests/c/test_slab_entry.cpp): both fields round-trip at their edges, no valid entry equals
the padding marker, and the narrow format is chosen exactly for ids below 2^26 - 1."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="no g++")
def test_slab_entry_formats(tmp_path):
    exe = tmp_path / "test_slab_entry"
    subprocess.run([GXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(ROOT, "emqx_amd/csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests/c/test_slab_entry.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
