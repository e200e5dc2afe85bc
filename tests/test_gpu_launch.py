"""lm_launch (csrc/launch.h), the one way the library launches a kernel, alone on the GPU (`-m gpu`): tests/cpp/launch_cases.cpp is built
next to the header and run once.  The rule around it — every launcher returns a checked status — is held by tests/test_launch_rule.py."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_helper_alone(tmp_path):
    """One 64-thread kernel that writes its arguments to a 64-byte buffer.  An int for an unsigned, a double for a float, a const T& for
    a 160-byte struct by value and a templated kernel instance arrive as `<<< >>>` delivers them; a launch of 2048 threads per block
    returns an error and the next launch on the stream returns hipSuccess and runs; a launch directly after an event query that may
    answer hipErrorNotReady returns hipSuccess."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "launch_cases")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "6dpose_amd", "csrc"), "-x", "hip", os.path.join(ROOT, "tests", "cpp", "launch_cases.cpp"), "-o", exe],
                          timeout=600)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert r.returncode == 0 and b"ok:" in r.stdout, r.stdout.decode()[-2000:]
