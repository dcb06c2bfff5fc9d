"""scs_hip_refine_batch / scs_hip_refine_batch_device consumed from plain C: tests/cabi/cabi_refine_batch.c."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "scs-python_amd", "scs")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _compile(tmp_path):
    exe = str(tmp_path / "cabi_refine_batch")
    cmd = ["gcc", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROCM, "include"),
           os.path.join(ROOT, "tests", "cabi", "cabi_refine_batch.c"), "-L", LIBDIR, "-lscs_hip", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
           "-lm", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_refine_batch_consumer_compiles_and_links(tmp_path):
    """CPU: the new declarations are valid C and resolve against libscs_hip.so; without a GPU the program says so and exits 2."""
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 2), out.stdout + out.stderr


@pytest.mark.gpu
def test_refine_batch_consumer_matches_three_solo_calls(tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout and "FAIL" not in out.stdout.replace("FAILED", ""), out.stdout
    assert out.stdout.count("identical") >= 15 and "member 2" in out.stdout and "no solve yet" in out.stdout, out.stdout
