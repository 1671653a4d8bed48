"""The host side of the priority mqueue stage (emqx_amd/csrc/pmqueue.cpp, pmqueue.h) built without a device
together with its stand-alone program (tests/c/test_pmqueue_host.cpp) and run on the CPU: once plainly,
once under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="no g++")
@pytest.mark.parametrize("sanitize", [False, True])
def test_pmqueue_host(tmp_path, sanitize):
    exe = tmp_path / "test_pmqueue_host"
    cmd = [GXX, "-std=c++17", "-O1" if sanitize else "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
           "-DEMQX_PMQUEUE_NO_DEVICE", "-o", str(exe),
           os.path.join(ROOT, "tests/c/test_pmqueue_host.cpp"), os.path.join(ROOT, "emqx_amd/csrc/pmqueue.cpp")]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    assert "pmqueue host ok" in out.stdout
