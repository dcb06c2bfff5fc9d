"""Device equilibration (K12: csrc/normalize_dev.hpp k_rescale_norm3 / k_pass_finish, driven by device_normalize in
csrc/device_csr.hpp) against the independent reference tests/equilibrate_ref.py at the edges of the kernels: the 64-row boundary of the
block reduction, one-row blocks, triples, rows / columns / lines of P beyond 2048 nonzeros, the 1024-row cap of a row block, both clamps,
empty lines, no separable prefix, no block at all, no nonzero at all, and the one-block-per-cone rule of the spectral cones
(tests/equilibrate_cases.py).  tests/test_equilibrate_ref_cpu.py proves the reference itself without a GPU."""
import functools

import numpy as np
import pytest

import equilibrate_cases as cases
import equilibrate_ref as ref
import spectral_ref

pytestmark = pytest.mark.gpu

RTOL = 1e-13  # the bound of test_equilibration_matches_oracle; >= 50 x the float64-against-longdouble floor (test_equilibrate_ref_cpu.py)
MIN_CLAMP_MARGIN = 1e-3
ULPS = 60  # A_hat[p] against A[p] D[i] E[j]: 26 passes of two roundings each, plus room
FIELDS = ("A", "P", "b", "c", "D", "E")


@pytest.fixture(scope="module")
def hip():
    from scs import _scs_hip
    assert _scs_hip.device_count() > 0, "GPU tests need a HIP device (no CPU fallback exists)"
    return _scs_hip


@pytest.fixture(scope="module")
def oracle():
    from oracle import scs_oracle
    return scs_oracle


@functools.lru_cache(maxsize=None)
def reference(name, with_P):
    cs = cases.case(name)
    return ref.equilibrate(cs["A"], cs["P"] if with_P else None, cs["b"], cs["c"], cs["cone"])


def rel_dev(got, want):
    """largest elementwise relative deviation; an exact zero must meet an exact zero"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0), "exact zeros differ"
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def worst_dev(got, want):
    """(worst relative deviation over A, P, b, c, D, E, sigma; the field it was seen in); got, want: (A, P, b, c, D, E, sigma)"""
    devs = [(rel_dev(g, w), f) for f, g, w in zip(FIELDS, got[:6], want[:6]) if w is not None]
    devs.append((rel_dev([got[6]], [want[6]]), "sigma"))
    return max(devs)


@pytest.mark.parametrize("with_P", [True, False], ids=["P", "noP"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_device_equilibration_at_the_edges(hip, oracle, name, with_P):
    """D, E, A_hat, P_hat, b_hat, c_hat and sigma of one call within 1e-13 (elementwise relative, zeros exact) of the float64
    reference and, where the CPU checker knows the cone, of the checker; D bit-constant on every block; the scaled values equal to
    the inputs times the scalings within 60 ulp; all scalings finite and positive; a second call returns the same bits.
    Seen on the device: at most 2.2e-15 from the reference (kitchen with P, in P_hat) and 4.8e-15 from the checker (long with P),
    next to a float64-against-longdouble floor of 2.0e-15."""
    cs = cases.case(name)
    A, P, b, c, cone = cs["A"], (cs["P"] if with_P else None), cs["b"], cs["c"], cs["cone"]
    want = reference(name, with_P)
    tag = "%s %s" % (name, "with P" if with_P else "no P")

    # conditions on the inputs: the limit jumps at its thresholds, and the block table must be the front end's
    assert want.clamp_margin >= MIN_CLAMP_MARGIN, (tag, want.clamp_margin)
    assert ref.table_rows(want.blocks) == spectral_ref.m_of(cone) == cs["rows"] == A.shape[0]

    entry = hip.normalize_spectral if cs["spectral"] else hip.normalize
    got = entry(A, P, b, c, cone)
    assert (got[1] is None) == (not with_P)

    dev, where = worst_dev(got, want[:7])
    print("equilibration %s: worst relative deviation from the float64 reference %.2e (%s)" % (tag, dev, where))
    if cs["spectral"]:
        odev = None  # the CPU checker has no spectral cones: the independent reference alone holds this case
    else:
        odev, owhere = worst_dev(got, oracle.normalize(A, P, b, c, cone)[:7])
        print("equilibration %s: worst relative deviation from the CPU checker %.2e (%s)" % (tag, odev, owhere))

    # independent of any reference
    Ah, Ph, D, E = got[0], got[1], got[4], got[5]
    assert np.all(np.isfinite(D)) and np.all(D > 0) and np.all(np.isfinite(E)) and np.all(E > 0), tag
    for at, ln in want.blocks[1]:
        assert np.all(D[at:at + ln] == D[at]), (tag, "D varies inside the block at row %d of length %d" % (at, ln))
    eps = np.finfo(np.float64).eps
    aj = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    prod = A.data * D[A.indices] * E[aj]
    assert np.all(np.abs(Ah - prod) <= ULPS * eps * np.abs(prod)), tag
    if with_P:
        pj = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
        prod = P.data * E[P.indices] * E[pj]
        assert np.all(np.abs(Ph - prod) <= ULPS * eps * np.abs(prod)), tag
    if name == "tiny_zero":
        assert np.all(D == 1.0) and np.all(E == 1.0) and got[6] == 1.0

    assert dev <= RTOL, (tag, where, dev)
    if odev is not None:
        assert odev <= RTOL, (tag, owhere, odev)

    # every reduction has a fixed order: a second call returns the same bits
    again = entry(A, P, b, c, cone)
    for f, g, h in zip(FIELDS + ("sigma",), got, again):
        if g is not None:
            assert np.array_equal(np.asarray(g), np.asarray(h)), (tag, f)
