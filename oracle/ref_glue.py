"""oracle/_ref: the reference's own CPython glue (scs/scspy.c with scsmodule.h / scsobject.h), compiled unchanged against this
repository's include/ and linked against libscs_hip.so (tests/test_reference_glue_cpu.py loads it).

build() runs this where the reference tree is present (SCS_REFERENCE_DIR, default: the build container's copy).  Only the compiled
module and the compiler's log land in oracle/_ref/, which git ignores; nothing of the reference enters the repository.  Without a
reference tree nothing is written, and the tests that need the module skip.  A glue that no longer compiles is not a build error:
the log keeps the compiler's message and the tests fail with it."""
import os
import subprocess
import sys
import sysconfig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(os.environ.get("SCS_REFERENCE_DIR", "/root/reference"), "scs")
OUT = os.path.join(HERE, "_ref")
MODULE = os.path.join(OUT, "_scs_direct" + sysconfig.get_config_var("EXT_SUFFIX"))   # default module name, R:scs/scsmodule.h:98-99
LOG = os.path.join(OUT, "scspy_build.log")
LIBDIR = os.path.join(ROOT, "scs-python_amd", "scs")


def build():
    """compile the glue into oracle/_ref; True when the module was built, False when it failed, None without a reference tree"""
    src = os.path.join(REF, "scspy.c")
    if not os.path.exists(src):
        return None
    import numpy as np
    os.makedirs(OUT, exist_ok=True)
    if os.path.exists(MODULE):
        os.remove(MODULE)
    cmd = ["gcc", "-shared", "-fPIC", "-O1", "-Werror=implicit-function-declaration", "-o", MODULE, src,
           "-I", os.path.join(ROOT, "include"), "-idirafter", os.path.join(HERE, "ref_compat"),
           "-I", sysconfig.get_paths()["include"], "-I", np.get_include(),
           "-DCTRLC=1", "-DCOPYAMATRIX=1",      # the defines every backend target passes, R:meson.build:288-313
           "-L", LIBDIR, "-lscs_hip", "-Wl,-rpath,$ORIGIN/" + os.path.relpath(LIBDIR, OUT)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    with open(LOG, "w") as f:
        f.write(" ".join(cmd) + "\n" + r.stdout + r.stderr + "exit %d\n" % r.returncode)
    return r.returncode == 0


if __name__ == "__main__":
    sys.exit(0 if build() is not False else 1)
