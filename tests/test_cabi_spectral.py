"""tests/cabi/cabi_spectral.c: a plain-C consumer compiled with -DUSE_SPECTRAL_CONES against include/ solves an ell1 + log-det
problem through plain scs_init (the header routes it to the spectral-aware entry: INTEGRATION.md §B)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "scs-python_amd", "scs")


def _compile(tmp_path):
    exe = str(tmp_path / "cabi_spectral")
    cmd = ["gcc", "-O2", "-DUSE_SPECTRAL_CONES", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi", "cabi_spectral.c"),
           "-L", LIBDIR, "-lscs_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-lm", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_spectral_consumer_compiles_and_links(tmp_path):
    """CPU: the header is valid C with the flag, and the remapped names resolve against libscs_hip.so"""
    exe = _compile(tmp_path)
    syms = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "scs_init_spectral" in syms
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode in (0, 2), out.stdout + out.stderr


@pytest.mark.gpu
def test_spectral_consumer_solves_on_device(tmp_path):
    exe = _compile(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout, out.stdout
