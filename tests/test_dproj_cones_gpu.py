"""W = D Pi_K(v) applied to a vector on the device for the box cone and the power cones (csrc/dproj_box_pow.hpp), through the one-shot
entry `_scs_hip.dproj_cone`, against the numpy reference of tests/dproj_cones_ref.py.

Box cone, k bound rows: the device forms dt = (u0 + sum a_j r_j) / h with ONE fixed-order sum of k products, so an entry of W u errs,
relative to the block norm |u|, by at most  4 k 2^-52 sum|a_j r_j| / (h |u|) + 2^-50  — the bound of a length-k sum (the tree the
device uses does much better) plus the roundings of u0, the division and the product a_j dt (|a_j| / h <= 1/2).  The reference's own
sum is exact (math.fsum of the rounded products).  Free rows are copied: exact.

Power cones: the 3 x 3 block comes from M = (I - mu H)^{-1} at the projected point, so its relative error is cond2(I - mu H) times the
rounding of a few dozen operations, once r is known to double precision: per cone |W u - ref| / |u| <= 64 cond2(I - mu H) 2^-52, the
condition number taken from the reference."""
import math

import numpy as np
import pytest

import adjoint_psd_ref as pr
import dproj_cones_ref as dr

from scs import _scs_hip

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MULTI_MIN = 16384  # csrc/cones.hpp kBoxMultiMin = csrc/dproj_box_pow.hpp kDboxMultiMin: bsize = k + 1 above it takes the two-launch form
# every lane count around a wavefront and around the 1024-lane workgroup, a cone past several strides, the threshold -1 / +0 / +1, and
# one size beyond the 256 workgroups x 256 lanes x 4 rows the multi-launch grid is capped at
BOX_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4100, MULTI_MIN - 2, MULTI_MIN - 1, MULTI_MIN, MULTI_MIN + 1, 300001]
MODES = {"pos": (), "zero": (), "noU": ("U",), "noL": ("L",)}


def box_reference(v, bl, bu, u):
    """(W u, the bound on its entries' error relative to |u|, (t*, U, L))"""
    t, a, act, h = dr.box_coef(v, bl, bu)
    prods = a[act] * u[1:][act]
    dt = (u[0] + math.fsum(prods)) / h if t > 0 else 0.0
    ref = np.concatenate([[dt], np.where(act, a * dt, u[1:])])
    k = v.size - 1
    bound = 4 * k * EPS * np.abs(prods).sum() / (h * np.linalg.norm(u)) + 2.0 ** -50
    return ref, bound, (t, act)


@pytest.mark.parametrize("k", BOX_SIZES)
def test_box_apply_matches_the_reference(k):
    seen_inf = seen_zero_active = False
    for i, (mode, empty) in enumerate(MODES.items()):
        rng = np.random.default_rng(1000 * i + k % 997)
        tstar = 0.0 if mode == "zero" else rng.uniform(0.5, 1.5)
        v, bl, bu = dr.box_case(rng, k, tstar, empty=empty)
        u = rng.standard_normal(k + 1)
        cone = {"bl": bl, "bu": bu}
        wu, wmiu = _scs_hip.dproj_cone(v, u, cone)
        again = _scs_hip.dproj_cone(v, u, cone)
        assert np.array_equal(wu, again[0]) and np.array_equal(wmiu, again[1])  # two calls: equal bits
        assert np.array_equal(wmiu, wu - u)
        ref, bound, (t, act) = box_reference(v, bl, bu, u)
        _, U, L = dr.box_sets(v, bl, bu, t)  # the case the generator built is the case the reference sees
        if mode == "zero":
            assert t == 0.0 and wu[0] == 0.0 and not wu[1:][act].any()
        else:
            assert abs(t - tstar) <= 1e-9 * max(1.0, abs(v[0]))
            if k >= 3:
                assert (mode == "noU") == (not U.any()) and (mode == "noL") == (not L.any()), (mode, U.sum(), L.sum())
        err = np.abs(wu - ref).max() / np.linalg.norm(u)
        print("box k = %d %s: t* = %.3f, %d active, entry error / |u| %.2e, bound %.2e" % (k, mode, t, act.sum(), err, bound))
        assert err <= bound, (k, mode, err, bound)
        assert np.array_equal(wu[1:][~act], u[1:][~act])  # free rows are copied
        seen_inf |= bool((~np.isfinite(bu)).any() and (~np.isfinite(bl)).any())
        zero_rows = act & (bl == 0) & (v[1:] < 0)
        if zero_rows.any():  # an active zero bound is not a free row: its output is 0, not r_j
            seen_zero_active = True
            assert not wu[1:][zero_rows].any() and u[1:][zero_rows].all()
    if k >= 3:
        assert seen_inf and seen_zero_active


POW_A = (0.1, 0.5, 0.9, -0.3, -0.5)
POW_N = 700  # more than two workgroups of 256 lanes, plus a tail
_pow = {}


def pow_inputs():
    """700 cones: exponent and case cycle independently (5 x 3 combinations), both signs of z by the generator's coin"""
    if not _pow:
        rng = np.random.default_rng(77)
        a = np.array([POW_A[i % 5] for i in range(POW_N)])
        case = [("in", "polar", "bd")[(i // 5) % 3] for i in range(POW_N)]
        v = np.concatenate([dr.pow_point(rng, a[i], case[i]) for i in range(POW_N)])
        u = rng.standard_normal(3 * POW_N)
        ref = np.concatenate([dr.pow_W(v[3 * i:3 * i + 3], a[i]) @ u[3 * i:3 * i + 3] for i in range(POW_N)])
        cond = np.array([dr.pow_cond(v[3 * i:3 * i + 3], a[i]) for i in range(POW_N)])
        _pow.update(a=a, case=case, v=v, u=u, ref=ref, cond=cond)
    return _pow


def test_pow_apply_matches_the_reference():
    d = pow_inputs()
    a, case, v, u = d["a"], d["case"], d["v"], d["u"]
    cone = {"p": a}
    wu, wmiu = _scs_hip.dproj_cone(v, u, cone)
    again = _scs_hip.dproj_cone(v, u, cone)
    assert np.array_equal(wu, again[0]) and np.array_equal(wmiu, again[1])
    assert np.array_equal(wmiu, wu - u)
    V, U3, W3, R3 = v.reshape(-1, 3), u.reshape(-1, 3), wu.reshape(-1, 3), d["ref"].reshape(-1, 3)
    err = np.linalg.norm(W3 - R3, axis=1) / np.linalg.norm(U3, axis=1)
    bound = 64 * d["cond"] * EPS
    worst = int(np.argmax(err / bound))
    print("pow: worst error / bound %.3f at cone %d (a = %g, %s, cond %.2f, error %.2e)" % (err[worst] / bound[worst], worst, a[worst], case[worst],
                                                                                         d["cond"][worst], err[worst]))
    assert (err <= bound).all(), (worst, a[worst], case[worst], err[worst], bound[worst])
    # the cases asserted really occur: every exponent in every case, both signs of z in every case, I and 0 exactly
    seen = {(a[i], case[i]) for i in range(POW_N)}
    assert seen == {(x, c) for x in POW_A for c in ("in", "polar", "bd")}
    for c in ("in", "polar", "bd"):
        signs = {np.sign(V[i, 2]) for i in range(POW_N) if case[i] == c}
        assert signs == {-1.0, 1.0}, (c, signs)
    for i in range(POW_N):
        assert dr.pow_case_of(V[i], a[i]) == case[i]
        if case[i] == "in":
            assert np.array_equal(W3[i], U3[i])
        elif case[i] == "polar":
            assert not W3[i].any()
        else:
            assert W3[i].any() and not np.array_equal(W3[i], U3[i])
    assert d["cond"].max() > 1.5  # the bound's factor is exercised


def test_every_cone_keeps_its_bits_next_to_the_others():
    """z | l | box | q | s | p in one call: every block is written at its own rows, with the bits of the block served alone"""
    rng = np.random.default_rng(8)
    d = pow_inputs()
    vb, bl, bu = dr.box_case(rng, 70, 0.9)
    q, s = [3, 9, 70], [3, 5]
    head = np.concatenate([rng.standard_normal(2), rng.standard_normal(5)])
    vq, vs = rng.standard_normal(sum(q)), np.concatenate([pr.psd_point(rng, 3, 1), pr.psd_point(rng, 5, 3)])
    np_ = 40
    vp, a = d["v"][:3 * np_], d["a"][:np_]
    v = np.concatenate([head, vb, vq, vs, vp])
    u = rng.standard_normal(v.size)
    cone = {"z": 2, "l": 5, "bl": bl, "bu": bu, "q": q, "s": s, "p": a}
    wu, wmiu = _scs_hip.dproj_cone(v, u, cone)
    assert np.array_equal(wmiu, wu - u)
    o = 0
    for part, sub in ((head, {"z": 2, "l": 5}), (vb, {"bl": bl, "bu": bu}), (np.concatenate([vq, vs]), {"q": q, "s": s}), (vp, {"p": a})):
        alone = _scs_hip.dproj_cone(part, u[o:o + part.size], sub)[0]
        assert np.array_equal(alone, wu[o:o + part.size]), sorted(sub)
        o += part.size
    assert o == v.size
    ref = dr.cone_W(v, cone) @ u
    # the row order: the blocks' own bounds are above and in the tests of the other cones; the loosest is the PSD blocks' — their
    # decomposition stops at a relative off-diagonal norm 1e-13 (adjoint_psd_ref.TAU) and the spectra keep a sign gap >= 0.1: 1e-12
    assert np.abs(wu - ref).max() <= 10 * pr.TAU / pr.GAP * np.linalg.norm(u)


def test_the_cones_without_a_derivative_are_still_refused_by_name():
    for cone, name, ln in (({"l": 1, "ep": 1}, r"exponential \(ep\) cone", 4), ({"l": 1, "ed": 1}, r"dual exponential \(ed\) cone", 4),
                           ({"l": 2, "cs": [2]}, r"complex PSD \(cs\) cone.*z, l, q and s cones only", 6)):
        with pytest.raises(RuntimeError, match=name):
            _scs_hip.dproj_cone(np.ones(ln), np.ones(ln), cone)
