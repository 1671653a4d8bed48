"""The host-only half of what the six session stages share (emqx_amd/csrc/stage_host.h with
EMQX_STAGE_NO_DEVICE: Stage, offsets_ok, stats_copy, create and destroy of a host-only handle, the
stubs of the device entry points) built with a plain C++ compiler together with its stand-alone
program (tests/c/test_stage_host.cpp) and run on the CPU: once plainly, once under AddressSanitizer
and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="no g++")
@pytest.mark.parametrize("sanitize", [False, True])
def test_stage_host(tmp_path, sanitize):
    exe = tmp_path / "test_stage_host"
    cmd = [GXX, "-std=c++17", "-O1" if sanitize else "-O2", "-Wall", "-Wextra", "-Werror", "-pthread",
           "-o", str(exe), os.path.join(ROOT, "tests/c/test_stage_host.cpp")]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    assert "stage host ok" in out.stdout
