"""the reference's OWN CPython glue (`scs/scspy.c` with `scsmodule.h` / `scsobject.h`) compiles against this
repo's `include/` (glbopts.h, scs.h, scs_types.h) and links against `libscs_hip.so` — unchanged.  build() compiles it into
oracle/_ref/ (oracle/ref_glue.py: nothing of the reference enters the repo); skipped where build() had no reference tree to compile.

The only local piece is a backport header for three CPython 3.13 functions the glue takes from the `pythoncapi-compat` submodule
(empty in the snapshot; `R:scs/scsobject.h:1,112,154,168`): oracle/ref_compat/.
Without a GPU `scs_init` returns NULL, so what can run here is everything the glue does BEFORE the core is entered
plus the failure path: module surface, argument parsing and its messages, and "ScsWork allocation error!".
"""
import importlib.util
import os

import numpy as np
import pytest
from scipy import sparse

from oracle import ref_glue

pytestmark = pytest.mark.skipif(not os.path.exists(ref_glue.LOG),
                                reason="oracle/_ref has no build of the reference glue: build() found no reference tree")


def _build_log():
    with open(ref_glue.LOG) as f:
        return f.read()[-3000:]


def test_reference_glue_compiles_against_include():
    """build() compiled the glue with -Werror=implicit-function-declaration (it recompiles it every time): every type, field,
    macro and function it names exists in include/."""
    assert os.path.exists(ref_glue.MODULE), _build_log()


@pytest.fixture(scope="module")
def glue():
    assert os.path.exists(ref_glue.MODULE), _build_log()
    from scs import _scs_hip  # noqa: F401  (preloads the HIP runtime the library links against)
    spec = importlib.util.spec_from_file_location("_scs_direct", ref_glue.MODULE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _args(m=2, n=1):
    A = sparse.csc_matrix(np.array([[1.0], [-1.0]]))
    return [(m, n), A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), None, None, None,
            np.array([1.0, 0.0]), np.array([1.0]), {"l": 2}]


def test_reference_glue_links_and_reports_this_library(glue):
    import scs
    assert glue.version() == scs.__version__          # scs_version() of libscs_hip.so through R:scs/scsmodule.h:5
    assert glue.sizeof_int() == 4 and glue.sizeof_float() == 8
    assert hasattr(glue, "SCS")


def test_reference_glue_argument_checks_run_before_the_core(glue):
    a = _args()
    a[7] = np.array([1.0, 0.0, 3.0])
    with pytest.raises(ValueError, match="b has incompatible dimension with A"):      # R:scs/scsobject.h:675
        glue.SCS(*a, verbose=False)
    a = _args()
    a[9] = {"l": 2, "q": [-1]}
    with pytest.raises(ValueError):                                                     # parse_pos_scs_int, :169
        glue.SCS(*a, verbose=False)
    with pytest.raises(TypeError):                                                      # PyArg table, :498-551
        glue.SCS(*_args(), max_iters="many")


def test_reference_glue_init_reaches_scs_init(glue):
    """With a device this constructs a workspace (the GPU suite drives the same C-ABI through ctypes and the plain-C
    consumer tests/cabi/cabi_smoke.c); without one scs_init returns NULL and the glue reports it: R:scs/scsobject.h:903-914."""
    from scs import _scs_hip
    if _scs_hip.device_count() > 0:
        s = glue.SCS(*_args(), verbose=False, eps_abs=1e-9, eps_rel=1e-9)
        sol = s.solve(False, None, None, None)
        assert sol["info"]["status"] == "solved" and abs(sol["x"][0]) < 1e-6
    else:
        with pytest.raises(ValueError, match="ScsWork allocation error"):
            glue.SCS(*_args(), verbose=False)
