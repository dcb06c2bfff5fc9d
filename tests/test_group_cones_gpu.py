"""Grouped solve (csrc/batch.hpp) of members with spectral cones, SOCs longer than kSocBig and small complex PSD cones.

Such members used to be solved one by one through scs_solve.  Now they share the launches of their group like any other
member: the contract is the one of tests/test_group_gpu.py — each member's answer is EXACTLY that of a solve of its own (same bits
in x, y, s, same iteration / CG-step / Anderson counters) — and scs.batch_plan reports the grouping solve_batch then runs."""
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

import spectral_ref as sr

pytestmark = pytest.mark.gpu

EXACT_INFO = ("status_val", "iter", "cg_iters", "scale_updates", "scale", "pobj", "dobj", "res_pri", "res_dual", "gap",
              "comp_slack", "rejected_accel_steps", "accepted_accel_steps")


def _assert_same(a, b, tag):
    for key in ("x", "y", "s"):
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (tag, key)
    for key in EXACT_INFO:
        va, vb = a["info"][key], b["info"][key]
        assert va == vb or (va != va and vb != vb), (tag, key, va, vb)
    assert a["info"]["aa_stats"] == b["info"]["aa_stats"], (tag, a["info"]["aa_stats"], b["info"]["aa_stats"])
    assert a["info"]["status"] == b["info"]["status"]


def _feasible_qp(cone, seed):
    """R:test/test_spectral_and_complex_cones.py:54-69 (as tests/test_spectral_cones_gpu.py generates it)"""
    rng = np.random.RandomState(seed)
    m = sr.m_of(cone)
    A = sp.random(m, m, density=0.5, format="csc", random_state=rng)
    A.data = rng.randn(A.nnz)
    c = rng.randn(m)
    b = A @ rng.randn(m) + np.abs(rng.randn(m))
    return dict(P=sp.eye(m, format="csc"), A=A, b=b, c=c)


def _projection_qp(cone, seed):
    """min 1/2 |z - w|^2 s.t. z in K: few nonzeros however long the cone"""
    L = sr.m_of(cone)
    w = np.random.default_rng(seed).standard_normal(L)
    return dict(P=sp.eye(L, format="csc"), A=-sp.eye(L, format="csc"), b=np.zeros(L), c=-w)


def _solo_and_group(problems, settings):
    """problems: list of (data, cone).  Separate solves and one solve_batch, each on fresh workspaces."""
    import scs
    solo = [scs.SCS(d, K, verbose=False, **settings).solve(warm_start=False) for d, K in problems]
    solvers = [scs.SCS(d, K, verbose=False, **settings) for d, K in problems]
    plan = scs.batch_plan(solvers)
    grp = scs.solve_batch(solvers, warm_start=False)
    return solo, grp, solvers, plan


def _check_group(problems, settings, tag):
    solo, grp, solvers, plan = _solo_and_group(problems, settings)
    assert plan == [0] * len(problems), (tag, plan)
    for i, (a, b) in enumerate(zip(solo, grp)):
        _assert_same(a, b, "%s member %d" % (tag, i))
        assert "grouped solve of %d" % len(problems) in b["info"]["lin_sys_solver"], b["info"]["lin_sys_solver"]
    return solo, grp, solvers


KITCHEN = dict(z=1, l=2, q=[3], s=[2], ep=1, d=[2], nuc_m=[3], nuc_n=[2], ell1=[3], sl_n=[3], sl_k=[1])


# ---------------------------------------------------------------- the plan
def test_plan_groups_spectral_long_soc_and_complex_psd_members():
    import scs
    batches = [[(_feasible_qp(KITCHEN, 100 + i), KITCHEN) for i in range(16)],
               [(_projection_qp({"l": 2, "q": [5000]}, 200 + i), {"l": 2, "q": [5000]}) for i in range(8)],
               [(_feasible_qp({"cs": [3, 5]}, 300 + i), {"cs": [3, 5]}) for i in range(8)]]
    for probs in batches:
        solvers = [scs.SCS(d, K, verbose=False) for d, K in probs]
        assert scs.batch_plan(solvers) == [0] * len(probs), probs[0][1]
    # what stays solo: a PSD matrix above order 32, a complex PSD cone whose embedding is (2k > 32)
    for K in ({"l": 2, "s": [40]}, {"l": 2, "cs": [17]}):
        solvers = [scs.SCS(_projection_qp(K, 400 + i), K, verbose=False) for i in range(2)]
        assert scs.batch_plan(solvers) == [-1, -1], K
    assert scs.batch_plan([]) == []
    sv = scs.SCS(*batches[0][0], verbose=False)
    with pytest.raises(ValueError, match="twice"):
        scs.batch_plan([sv, sv])
    with pytest.raises(TypeError):
        scs.batch_plan([sv._solver])


# ---------------------------------------------------------------- bit identity, family by family
FAMILIES = [
    ("ell1_short", {"l": 2, "ell1": [7, 3]}, "qp", 3),
    ("ell1_long", {"l": 2, "ell1": [4097]}, "proj", 3),
    ("sl", {"l": 2, "sl_n": [4, 3], "sl_k": [2, 3]}, "qp", 3),            # (k = n in the second cone)
    ("d", {"l": 2, "d": [1, 3]}, "qp", 3),
    ("d64", {"d": [64]}, "proj", 2),
    ("nuc_small", {"l": 1, "nuc_m": [3, 2], "nuc_n": [2, 3]}, "qp", 3),
    ("nuc_largest", {"nuc_m": [128], "nuc_n": [64]}, "proj", 2),
    ("soc_long", {"l": 3, "q": [4, 5000]}, "proj", 3),
    ("cs_mix", {"l": 3, "s": [3], "cs": [3, 2]}, "qp", 3),
]


@pytest.mark.parametrize("name,cone,gen,count", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_group_bit_identical_per_family(name, cone, gen, count):
    make = _feasible_qp if gen == "qp" else _projection_qp
    seed = zlib.crc32(name.encode()) % 100000
    probs = [(make(cone, seed + i), cone) for i in range(count)]
    _check_group(probs, dict(max_iters=2000), name)


# ---------------------------------------------------------------- variants on a mix of every family
MIX = dict(z=1, l=2, q=[3], s=[2], cs=[2], ep=1, d=[2], nuc_m=[3], nuc_n=[2], ell1=[3], sl_n=[3], sl_k=[1])


@pytest.mark.parametrize("settings", [dict(acceleration_type_1=True), dict(acceleration_type_1=False, acceleration_interval=1),
                                      dict(acceleration_lookback=0)], ids=["aa_type1", "aa_type2", "aa_off"])
def test_group_mix_acceleration_variants(settings):
    probs = [(_feasible_qp(MIX, 500 + i), MIX) for i in range(4)]
    _check_group(probs, dict(settings, max_iters=3000), str(settings))


def test_group_mix_warm_start_after_update():
    import scs
    probs = [(_feasible_qp(MIX, 600 + i), MIX) for i in range(3)]
    _, grp, solvers = _check_group(probs, dict(max_iters=3000), "cold")
    refs = [scs.SCS(d, K, verbose=False, max_iters=3000) for d, K in probs]
    solo2 = []
    for sv, rs, (d, K) in zip(solvers, refs, probs):
        rs.solve(warm_start=False)
        nb = d["b"] * 1.01
        sv.update(b=nb)
        rs.update(b=nb)
        solo2.append(rs.solve(warm_start=True))
    grp2 = scs.solve_batch(solvers, warm_start=True)
    for i, (a, b) in enumerate(zip(solo2, grp2)):
        _assert_same(a, b, "warm member %d" % i)
        assert b["info"]["iter"] <= grp[i]["info"]["iter"]


def test_group_mix_scale_updates_at_different_iterations():
    probs = []
    for i in range(4):
        d = _feasible_qp(MIX, 700 + i)
        d["b"] = d["b"] * (1e3 if i % 2 else 1e-3)
        d["A"] = d["A"] * (30.0 if i % 3 == 0 else 1.0)
        probs.append((d, MIX))
    solo, _, _ = _check_group(probs, dict(max_iters=1500, eps_abs=1e-9, eps_rel=1e-9), "scale updates")
    ups = [r["info"]["scale_updates"] for r in solo]
    assert any(u > 0 for u in ups) and len(set(ups)) > 1, ups


def _lp_members(cone, seed):
    """no P: a solved, an infeasible and an unbounded member of the same shape (certificates next to solutions)"""
    from scs import _scs_hip
    rng = np.random.default_rng(seed)
    m, n = sr.m_of(cone), 6
    out = []
    for kind in ("solved", "infeasible", "unbounded", "solved"):
        A = rng.standard_normal((m, n))
        z = rng.standard_normal(m)
        s = _scs_hip.proj_cone(z, cone)                 # s in K, y in K*, s'y = 0 (Moreau)
        y = _scs_hip.proj_cone(-z, cone, dual=True)
        s[:cone["z"]] = 0.0
        x = rng.standard_normal(n)
        if kind == "unbounded":
            A[:, 0] = 0.0                              # x_0 is free in the constraints and lowers the objective without end
        b = A @ x + s
        c = -A.T @ y
        if kind == "unbounded":
            c[0] = -1.0
        if kind == "infeasible":
            A[1] = A[0]                                # two zero-cone rows: a_0'x = b_0 and a_0'x = b_0 + 1
            b[1] = b[0] + 1.0
        out.append((dict(A=sp.csc_matrix(A), b=b, c=c), cone))
    return out


def test_group_mix_certificates():
    cone = dict(z=2, l=3, cs=[2], d=[2], nuc_m=[3], nuc_n=[2], ell1=[3], sl_n=[3], sl_k=[1])
    solo, _, _ = _check_group(_lp_members(cone, 800), dict(max_iters=5000), "certificates")
    assert {"infeasible", "unbounded"} <= {r["info"]["status"] for r in solo}, [r["info"]["status"] for r in solo]


# ---------------------------------------------------------------- shape rules
def _check_split(probs, expect_plan):
    import scs
    solo, grp, _, plan = _solo_and_group(probs, dict(max_iters=2000))
    assert plan == expect_plan, plan
    for i, (a, b) in enumerate(zip(solo, grp)):
        _assert_same(a, b, "member %d" % i)
        size = expect_plan.count(expect_plan[i])
        if expect_plan[i] >= 0:
            assert "grouped solve of %d" % size in b["info"]["lin_sys_solver"]
        else:
            assert "grouped" not in b["info"]["lin_sys_solver"]
    del scs


def test_members_that_differ_only_in_sl_k_do_not_share_a_group():
    Ka, Kb = {"l": 2, "sl_n": [4], "sl_k": [1]}, {"l": 2, "sl_n": [4], "sl_k": [2]}
    probs = [(_feasible_qp(K, 900 + i), K) for i, K in enumerate((Ka, Kb, Ka, Kb, Kb))]
    _check_split(probs, [0, 1, 0, 1, 1])


def test_members_that_differ_only_in_the_order_of_d_do_not_share_a_group():
    Ka, Kb = {"l": 1, "d": [2, 3]}, {"l": 1, "d": [3, 2]}
    probs = [(_feasible_qp(K, 1000 + i), K) for i, K in enumerate((Ka, Ka, Kb, Kb, Ka))]
    _check_split(probs, [0, 0, 1, 1, 0])


def test_two_spectral_shapes_and_a_large_psd_member():
    Ka, Kb, Kc = {"l": 2, "nuc_m": [3], "nuc_n": [2], "ell1": [4]}, {"l": 2, "sl_n": [3], "sl_k": [2], "cs": [2]}, {"l": 2, "s": [40]}
    probs = [(_feasible_qp(Ka, 1100), Ka), (_feasible_qp(Kb, 1101), Kb), (_projection_qp(Kc, 1102), Kc),
             (_feasible_qp(Ka, 1103), Ka), (_feasible_qp(Kb, 1104), Kb)]
    _check_split(probs, [0, 1, -1, 0, 1])


# ---------------------------------------------------------------- sharding on one GPU
def test_solve_sharded_spectral_batch_equals_solve_batch():
    import scs
    from scs import batch
    probs = [(_feasible_qp(KITCHEN, 1200 + i), KITCHEN, dict(verbose=False, max_iters=3000)) for i in range(4)]
    sharded = batch.solve_sharded(probs)
    grp = scs.solve_batch([scs.SCS(d, K, **st) for d, K, st in probs])
    for i, (a, b) in enumerate(zip(sharded, grp)):
        for key in ("x", "y", "s"):
            assert np.array_equal(a[key], b[key]), (i, key)
        assert a["info"]["iter"] == b["info"]["iter"] and a["info"]["status_val"] == b["info"]["status_val"]
