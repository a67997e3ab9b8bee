"""The launchers' typed dispatch header (torchseg_amd/csrc/tsg_dispatch.h), checked on the host (no GPU needed).

tests/dispatch_check.cpp is a stand-alone program with its own main: it is compiled host-only with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process.  It asserts, for every dispatcher and every accepted runtime
value, the tag the callable receives and that the callable's return value is passed through, and for values outside the
accepted set (dtype 2 and -1, label type 7, an int that is not in Ns...) that the callable is not called and the
documented error code comes back."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_dispatchers_pass_the_documented_tags(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "dispatch_check"
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "dispatch_check.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks passed" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr
