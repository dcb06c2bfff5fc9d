"""The independent equilibration reference (tests/equilibrate_ref.py) proved without a GPU: against the CPU checker's restatement
(oracle/oscs_normalize.c) on every non-spectral edge case of tests/equilibrate_cases.py, against its own longdouble run on all of
them, and on properties that need no second implementation.  tests/test_equilibrate_gpu.py then holds the device to this reference."""
import functools

import numpy as np
import pytest
from scipy import sparse

import equilibrate_cases as cases
import equilibrate_ref as ref
import spectral_ref

RTOL = 1e-14  # float64 reference against the checker and against longdouble, elementwise relative
GPU_RTOL = 1e-13  # what tests/test_equilibrate_gpu.py asks of the device
MIN_CLAMP_MARGIN = 1e-3
ULPS = 60  # A_hat[p] against A[p] D[i] E[j]: 26 passes of two roundings each, plus room
FIELDS = ("A", "P", "b", "c", "D", "E")


@pytest.fixture(scope="module")
def oracle():
    from oracle import scs_oracle
    return scs_oracle


@functools.lru_cache(maxsize=None)
def solved(name):
    """(name, case, reference with P, reference without P), computed once per case and shared by the tests"""
    cs = cases.case(name)
    return (name, cs, ref.equilibrate(cs["A"], cs["P"], cs["b"], cs["c"], cs["cone"]),
            ref.equilibrate(cs["A"], None, cs["b"], cs["c"], cs["cone"]))


every_case = pytest.mark.parametrize("name", cases.NAMES)
# the CPU checker has no spectral cones: that case is held by the longdouble run and the properties alone
checker_case = pytest.mark.parametrize("name", [n for n in cases.NAMES if not cases.case(n)["spectral"]])


def rel_dev(got, want):
    """largest elementwise relative deviation; an exact zero must meet an exact zero"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    assert got.shape == want.shape
    assert np.array_equal(got == 0, want == 0), "exact zeros differ"
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def worst_dev(got, want):
    """(worst relative deviation over A, P, b, c, D, E, sigma; the field it was seen in)"""
    devs = [(rel_dev(getattr(got, f), getattr(want, f)), f) for f in FIELDS if getattr(want, f) is not None]
    devs.append((rel_dev([got.sigma], [want.sigma]), "sigma"))
    return max(devs)


@every_case
def test_input_conditions(name):
    name, cs, with_p, without_p = solved(name)
    assert ref.table_rows(with_p.blocks) == spectral_ref.m_of(cs["cone"]) == cs["rows"] == cs["A"].shape[0]
    for r in (with_p, without_p):
        assert r.clamp_margin >= MIN_CLAMP_MARGIN, (name, r.clamp_margin)
    print("%s: clamp margin %.3g with P, %.3g without" % (name, with_p.clamp_margin, without_p.clamp_margin))


@checker_case
def test_reference_matches_the_checker(name, oracle):
    name, cs, with_p, without_p = solved(name)
    for r, P in ((with_p, cs["P"]), (without_p, None)):
        o = oracle.normalize(cs["A"], P, cs["b"], cs["c"], cs["cone"])
        want = ref.Equilibrated(*o[:7], blocks=None, clamp_margin=None, passes=None)
        dev, where = worst_dev(r, want)
        print("%s %s: worst deviation from the checker %.2e (%s)" % (name, "with P" if P is not None else "no P", dev, where))
        assert dev <= RTOL, (name, where, dev)


@every_case
def test_float64_matches_longdouble(name):
    name, cs, with_p, without_p = solved(name)
    for r, P in ((with_p, cs["P"]), (without_p, None)):
        hi = ref.equilibrate(cs["A"], P, cs["b"], cs["c"], cs["cone"], dtype=np.longdouble)
        dev, where = worst_dev(r, hi)
        print("%s %s: float64 against longdouble %.2e (%s)" % (name, "with P" if P is not None else "no P", dev, where))
        assert dev <= RTOL, (name, where, dev)
        # the device's bound (test_equilibrate_gpu.py) stays at least 50 times above this floor
        assert 50 * dev <= GPU_RTOL, (name, where, dev)


@every_case
def test_row_scale_is_constant_on_every_block(name):
    name, cs, with_p, without_p = solved(name)
    for r in (with_p, without_p):
        for at, ln in r.blocks[1]:
            assert np.all(r.D[at:at + ln] == r.D[at]), (name, at, ln)


@every_case
def test_scaled_values_are_the_inputs_times_the_scalings(name):
    name, cs, with_p, without_p = solved(name)
    A, P = cs["A"], cs["P"]
    aj = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    pj = np.repeat(np.arange(P.shape[1]), np.diff(P.indptr))
    eps = np.finfo(np.float64).eps
    for r in (with_p, without_p):
        want = A.data * r.D[A.indices] * r.E[aj]
        assert np.all(np.abs(r.A - want) <= ULPS * eps * np.abs(want)), name
        if r.P is not None:
            want = P.data * r.E[P.indices] * r.E[pj]
            assert np.all(np.abs(r.P - want) <= ULPS * eps * np.abs(want)), name


@every_case
def test_factors_stay_in_the_clamp_range(name):
    """limit(x) lies in [1e-4, 1e4], so a factor lies in [1e-2, 1e2]; a norm that was not clamped gives a factor strictly inside"""
    name, cs, with_p, without_p = solved(name)
    for r in (with_p, without_p):
        for dn, en, dt, et in r.passes:
            for x, f in ((dn, dt), (en, et)):
                assert np.all(np.isfinite(f)) and np.all(f >= 1e-2) and np.all(f <= 1e2), name
                free = (x > ref.LO) & (x < ref.HI)
                assert np.all((f[free] > 1e-2) & (f[free] < 1e2)), name
                assert np.all(f[x < ref.LO] == 1.0), name
        assert np.all(np.isfinite(r.D)) and np.all(r.D > 0) and np.all(np.isfinite(r.E)) and np.all(r.E > 0), name


def test_the_cases_reach_what_they_are_for():
    """the marked lines do what the case table says: both clamps fire, zero norms occur, rows and columns pass 2048 nonzeros"""
    k = ref.equilibrate(*[cases.case("kitchen")[key] for key in ("A", "P", "b", "c", "cone")])
    dn0, en0 = k.passes[0][0], k.passes[0][1]
    assert (dn0 > ref.HI).any() and (en0 > ref.HI).any() and (dn0 == 0).any() and (en0 == 0).any()
    assert ((dn0 > 0) & (dn0 < ref.LO)).any() and ((en0 > 0) & (en0 < ref.LO)).any()
    lengths = sorted(ln for _, ln in k.blocks[1])
    assert lengths[0] == 1 and 64 in lengths and 65 in lengths and 129 in lengths and 3 in lengths
    lg = cases.case("long")
    assert np.diff(lg["A"].indptr).max() > 2048 and np.diff(lg["A"].tocsr().indptr).max() > 2048
    full = (lg["P"] + sparse.triu(lg["P"], 1).T).tocsr()
    assert np.diff(full.indptr).max() > 2048
    rows_in_2100 = np.flatnonzero(np.diff(lg["A"].tocsr().indptr) > 2048)
    assert (rows_in_2100 < 47).any() and (rows_in_2100 >= 47 + 267).any()
    th = cases.case("thin")
    assert np.diff(th["A"].tocsr().indptr).max() <= 2 and th["A"].nnz < 2 * 3000
    assert ref.block_table(th["cone"]) == (3000, [])
    assert ref.block_table(cases.case("no_prefix")["cone"]) == (0, [(0, 2100)])
    assert len(ref.block_table(cases.case("many_blocks")["cone"])[1]) == 350
    assert cases.case("tiny_zero")["A"].nnz == 0
    z = ref.equilibrate(*[cases.case("tiny_zero")[key] for key in ("A", "P", "b", "c", "cone")])
    assert np.all(z.D == 1.0) and np.all(z.E == 1.0) and z.sigma == 1.0
    sp = ref.block_table(cases.case("spectral")["cone"])
    assert [ln for _, ln in sp[1]] == [3, 3, 17, 7, 71, 2, 101, 11, 67] and sp[0] == 2

