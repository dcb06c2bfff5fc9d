"""Problems and sequences of tests/test_pool_lifecycle_gpu.py, shared with the child processes it starts (the pool's cap and the
poison mode are read once per process).

A FAMILY is a function run(which) -> list of result dicts: it builds the workspaces of problem "A" or "B" (same shape: same cone,
same m, n and number of nonzeros; other data, another seed, another scale), solves, destroys every workspace it made and returns
what the solves returned.  Nothing of a family stays alive after run() returns, so the pool's account can be read exactly.

Sizes: a device buffer of at most 1 MiB lives in the workspace's arena, whose chunks are cleared whenever they are handed out, so
only LARGER buffers (and the buffers made while no arena is current: the dense inverse, the tables and staging of a grouped solve)
ever see a previous owner's data.  The solo families are therefore sized so that their vectors, matrices and cone scratch exceed
1 MiB (m > 131072 doubles, PSD matrices above order 362), at a few ADMM iterations each."""
import functools
import gc
import zlib

import numpy as np
import scipy.sparse as sp

import problem_gen as pg
import spectral_ref as sr

MiB = 1 << 20


def stats():
    from scs import _scs_hip
    return _scs_hip.pool_stats()


def trim():
    from scs import _scs_hip
    gc.collect()
    _scs_hip.trim_pool()


def nothing_lost(tag=""):
    """invariant 1 with no workspace alive: every byte obtained from the driver is in the pool"""
    gc.collect()
    st = stats()
    assert st["live_bytes"] == st["held_bytes"], (tag, st)
    return st


def same_bits(a, b, tag):
    for key in ("x", "y", "s"):
        assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs (max |diff| %r)" % (
            tag, key, float(np.nanmax(np.abs(a[key] - b[key]))))
    for key in ("iter", "status_val", "cg_iters", "scale_updates", "accepted_accel_steps", "rejected_accel_steps"):
        assert a["info"][key] == b["info"][key], (tag, key, a["info"][key], b["info"][key])


def _proj_dual(z, K):
    from scs import _scs_hip
    return _scs_hip.proj_cone(z, K, dual=True)


def _rescale(data, which):
    """problem B: other numbers (the caller used another seed) at another scale"""
    if which == "B":
        data = dict(data)
        data["b"] = data["b"] * 37.0
        data["c"] = data["c"] * 0.05
    return data


def _same_pattern(data, K, seed):
    """another problem on the sparsity patterns of `data` (the generators drop duplicate entries, so another seed alone would
    change the number of nonzeros and with it the sizes of the device buffers): new values, new primal-dual point"""
    rng = np.random.default_rng(seed)
    A = data["A"].copy()
    A.data = rng.standard_normal(A.nnz)
    m, n = A.shape
    z = rng.standard_normal(m)
    y = np.asarray(_proj_dual(z, K), dtype=np.float64)
    x = rng.standard_normal(n)
    out = {"A": A, "b": A @ x + (y - z), "c": -(A.T @ y)}
    if data.get("P") is not None:
        P = data["P"].copy()
        P.data = P.data * 2.5
        out["P"] = P
        out["c"] = out["c"] - (P + sp.triu(P, 1).T) @ x
    return out


@functools.lru_cache(maxsize=None)
def generated(name, which):
    """(data, cone) of the named generated problem; cached, so that no generation (it projects on the device) runs between the
    reads of the pool's counters"""
    seed = zlib.crc32(name.encode()) % 10000
    if which == "B":
        data, K = generated(name, "A")
        return _rescale(_same_pattern(data, K, seed + 1), "B"), K
    if name == "config5":
        K, n, k, _ = pg.workload("config5_small")
        data = pg.gen_feasible(K, n, k, 1000 + seed, _proj_dual)[0]
    elif name == "lp_soc_big":          # nnz = 360000: A, A' and every m-vector of the LP beyond the arena's limit
        K, n, k = {"l": 120000, "q": [10] * 2000}, 60000, 6
        data = pg.gen_feasible(K, n, k, seed, _proj_dual)[0]
    elif name == "mixed_big":           # z / l / box / q / exp / dual exp / power, m = 158000
        rng = np.random.default_rng(5)
        K = {"z": 10000, "l": 40000, "bu": rng.uniform(0.5, 2.0, 9999).tolist(), "bl": (-rng.uniform(0.5, 2.0, 9999)).tolist(),
             "q": [20] * 1000, "ep": 10000, "ed": 10000, "p": (rng.uniform(0.1, 0.9, 6000) * rng.choice([-1.0, 1.0], 6000)).tolist()}
        data = pg.gen_feasible(K, 60000, 8, seed, _proj_dual)[0]
    elif name == "psd_big":             # order 400: 1.28 MB per matrix buffer
        K = {"l": 100, "s": [400, 40, 5]}
        data = pg.gen_feasible(K, 3000, 30, seed, _proj_dual)[0]
    elif name == "cpsd_big":            # complex order 250: real embedding of order 500
        K = {"l": 100, "cs": [250, 3]}
        data = pg.gen_feasible(K, 3000, 30, seed, _proj_dual)[0]
    elif name == "qp_mid":              # n = 1350 with P: what the dense direct solver and a warm start are cycled on
        K, n, k, _ = pg.workload("config5_small")
        data = pg.gen_feasible_qp(K, n, k, seed, _proj_dual)[0]
    else:
        raise KeyError(name)
    return data, K


def projection_qp(cone, seed, scale=1.0):
    """min 1/2 |z - w|^2 s.t. z in K: P = I, A = -I (as tests/test_group_cones_gpu.py builds it)"""
    L = sr.m_of(cone)
    w = scale * np.random.default_rng(seed).standard_normal(L)
    return dict(P=sp.eye(L, format="csc"), A=-sp.eye(L, format="csc"), b=np.zeros(L), c=-w)


def feasible_qp(cone, seed, which="A"):
    """R:test/test_spectral_and_complex_cones.py:54-69 (as tests/test_spectral_cones_gpu.py generates it); B keeps A's pattern"""
    rng = np.random.RandomState(seed)
    m = sr.m_of(cone)
    A = sp.random(m, m, density=0.5, format="csc", random_state=rng)
    if which == "B":
        rng = np.random.RandomState(seed + 7919)
    A.data = rng.randn(A.nnz)
    c = rng.randn(m)
    b = A @ rng.randn(m) + np.abs(rng.randn(m))
    return _rescale(dict(P=sp.eye(m, format="csc"), A=A, b=b, c=c), which)


# one cone kind each, many cones: the m-vectors and the per-kind scratch exceed 1 MiB
SPECTRAL_BIG = {
    "logdet": {"l": 2, "d": [64] * 70},
    "nuclear": {"l": 2, "nuc_m": [128] * 20, "nuc_n": [64] * 20},
    "ell1": {"l": 2, "ell1": [70000, 70001]},
    "sum_largest": {"l": 2, "sl_n": [64] * 70, "sl_k": [7] * 70},
}
KITCHEN = dict(z=1, l=2, q=[3], s=[2], cs=[2], ep=1, d=[2], nuc_m=[3], nuc_n=[2], ell1=[3], sl_n=[3], sl_k=[1])


def _solve_solo(data, cone, settings, warm=False):
    import scs
    sv = scs.SCS(data, cone, verbose=False, **settings)
    out = [sv.solve(warm_start=False)]
    if warm:
        out.append(sv.solve(warm_start=True))
    del sv
    gc.collect()
    return out


def solo_family(name, settings, warm=False):
    def run(which):
        data, cone = generated(name, which)
        return _solve_solo(data, cone, settings, warm)
    return run


def spectral_family(kind):
    cone = SPECTRAL_BIG[kind]

    def run(which):
        data = projection_qp(cone, 11 if which == "A" else 12, 1.0 if which == "A" else 37.0)
        return _solve_solo(data, cone, dict(max_iters=12))
    return run


def _solve_group(problems, settings, expect_grouped=True):
    import scs
    solvers = [scs.SCS(d, K, verbose=False, **settings) for d, K in problems]
    if expect_grouped:
        assert scs.batch_plan(solvers) == [0] * len(solvers)
    out = scs.solve_batch(solvers, warm_start=False)
    del solvers
    gc.collect()
    return out


def group_family(cone, gen, count, settings):
    """a solve_batch group of `count` members of one cone (tests/test_group_cones_gpu.py FAMILIES)"""
    def run(which):
        base = zlib.crc32(repr(sorted(cone.items())).encode()) % 100000 + (0 if which == "A" else 50)
        if gen == "qp":
            probs = [(feasible_qp(cone, base + i, which), cone) for i in range(count)]
        else:
            probs = [(projection_qp(cone, base + i, 1.0 if which == "A" else 37.0), cone) for i in range(count)]
        return _solve_group(probs, settings)
    return run


@functools.lru_cache(maxsize=None)
def _config5_member(seed):
    K, n, k, _ = pg.workload("config5_small")
    return pg.gen_feasible(K, n, k, seed, _proj_dual)[0]


def config5_group(count, linear_solver, max_iters=20):
    def run(which):
        import scs
        K, n, k, seed = pg.workload("config5_small")
        probs = []
        for i in range(count):
            data = _config5_member(seed + i)
            probs.append((data if which == "A" else _rescale(_same_pattern(data, K, seed + i + 5000), "B"), K))
        return _solve_group(probs, dict(linear_solver=scs.LinearSolver(linear_solver), max_iters=max_iters))
    return run


def families():
    """name -> run(which); every family keeps ONE shape for A and B"""
    import test_group_cones_gpu as tg
    it = dict(max_iters=25)
    fam = {
        "lp_soc": solo_family("lp_soc_big", it),
        "exp_power_box": solo_family("mixed_big", it),
        "psd": solo_family("psd_big", dict(max_iters=10)),
        "complex_psd": solo_family("cpsd_big", dict(max_iters=10)),
        "hip_dense": solo_family("qp_mid", dict(linear_solver="hip_dense", max_iters=200)),
        "aa_type1": solo_family("lp_soc_big", dict(max_iters=60, acceleration_type_1=True)),
        "aa_type2": solo_family("lp_soc_big", dict(max_iters=60, acceleration_type_1=False, acceleration_interval=1)),
        "aa_off": solo_family("lp_soc_big", dict(max_iters=60, acceleration_lookback=0)),
        "warm_start": solo_family("lp_soc_big", dict(max_iters=30), warm=True),
        "warm_start_dense": solo_family("qp_mid", dict(linear_solver="hip_dense", max_iters=60), warm=True),
        "kitchen_solo": lambda which: _solve_solo(feasible_qp(KITCHEN, 7, which), KITCHEN, dict(max_iters=3000)),
        "group_config5_indirect": config5_group(8, "hip_indirect"),
        "group_config5_dense": config5_group(8, "hip_dense"),
    }
    for kind in SPECTRAL_BIG:
        fam["spectral_" + kind] = spectral_family(kind)
    for name, cone, gen, count in tg.FAMILIES:
        fam["group_" + name] = group_family(cone, gen, count, dict(max_iters=300))
    fam["group_mix"] = group_family(tg.MIX, "qp", 4, dict(max_iters=3000))
    return fam
