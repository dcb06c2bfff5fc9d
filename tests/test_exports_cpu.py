"""libscs_hip.so exports the C ABI of include/scs_hip.h and nothing else (the library used to export every
kernel stub and inline helper, 142 `T` + 664 `W` dynamic symbols for a few dozen functions)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "scs-python_amd", "scs", "libscs_hip.so")
HEADER = os.path.join(ROOT, "include", "scs_hip.h")
BINDINGS = os.path.join(ROOT, "scs-python_amd", "scs", "_scs_hip.py")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="libscs_hip.so is not built")


def declared_functions():
    """names of the functions the header declares (both parts, the spectral entries included)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    names = re.findall(r"\b(scs_\w+)\s*\(", text)
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
    return set(names)


def exported_functions():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    return {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in ("T", "W")}


def test_every_declaration_carries_the_export_macro():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tagged = set(re.findall(r"^SCS_HIP_API\b[^;(]*?\b(scs_\w+)\s*\(", text, flags=re.M))
    assert tagged == declared_functions()


def test_library_exports_exactly_the_declared_functions():
    declared, exported = declared_functions(), exported_functions()
    assert len(declared) >= 40, sorted(declared)  # (the parser found the header's declarations)
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))


def test_python_bindings_use_exported_functions_only():
    bound = set(re.findall(r"\blib\.(scs_\w+)", open(BINDINGS).read()))
    assert len(bound) >= 30, sorted(bound)
    assert bound <= exported_functions(), sorted(bound - exported_functions())
