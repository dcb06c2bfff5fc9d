"""Lifecycle of the device block pool (scs-python_amd/csrc/common.hpp DevPool) through its account `scs._scs_hip.pool_stats()`.

A workspace that dies hands its device blocks to the pool (only ~ScsHipWork does, once its stream is idle), and every allocation
looks there first (exact size, same device).  The counters are host integers kept under the pool's lock, so every relation below
is EXACT: no tolerance anywhere.  Other processes share the GPU, so nothing here reads hipMemGetInfo.

Every test starts from an empty pool (trim_pool), works with differences of the counters and destroys its workspaces (del +
gc.collect(): scs_finish runs from the wrapper's __del__) before it reads them.

What stays outside the pool on purpose: DevBufs released while their stream may still be busy — the scratch of scs_init's device
setup, the stack workspaces of the kernel-level entry points (proj_cone, spmv, kkt_solve), the tables a grouped solve frees when it
returns.  They are allocated through the same dev_malloc (so they may TAKE a pooled block) but return to the driver with hipFree,
whose implicit synchronisation is what makes that safe.  They are the `misses` that remain in a cycle on recycled blocks.

The cap (SCS_HIP_POOL_MB) and the poison mode (SCS_HIP_POOL_POISON, labs build) are read once per process: those tests run in a
child process each, under a timeout; a non-zero exit status fails the test and nothing more is started."""
import gc
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import pool_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _empty_pool():
    pc.trim()
    st = pc.stats()
    assert st["live_bytes"] == 0 and st["held_bytes"] == 0 and st["held_blocks"] == 0, st   # invariant 1, after trim_pool()
    yield
    pc.trim()


def _delta(a, b):
    return {k: b[k] - a[k] for k in ("hits", "misses")}


# ---------------------------------------------------------------- 1 + 2: nothing is lost, same-shape cycles reuse
def _cycle_shapes():
    import scs
    return {
        "config5_arena": lambda: (pc.generated("config5", "A"), dict(linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=20)),
        "exact_size_blocks": lambda: (pc.generated("lp_soc_big", "A"), dict(linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=20)),
        "hip_dense": lambda: (pc.generated("config5", "A"), dict(linear_solver=scs.LinearSolver.HIP_DENSE, max_iters=20)),
        "every_spectral_kind": lambda: ((pc.feasible_qp(pc.KITCHEN, 3), pc.KITCHEN), dict(max_iters=50)),
        "complex_psd": lambda: ((pc.feasible_qp({"l": 2, "cs": [3, 5]}, 4), {"l": 2, "cs": [3, 5]}), dict(max_iters=50)),
    }


@pytest.mark.parametrize("shape", ["config5_arena", "exact_size_blocks", "hip_dense", "every_spectral_kind", "complex_psd"])
def test_same_shape_cycles_reuse_every_pooled_block(shape):
    import scs
    (data, cone), settings = _cycle_shapes()[shape]()
    pc.trim()                       # (the generation above projected on the device)
    assert pc.stats()["live_bytes"] == 0
    after, per_cycle = [], []
    for k in range(5):
        before = pc.stats()
        sv = scs.SCS(data, cone, verbose=False, **settings)
        sv.solve(warm_start=False)
        alive = pc.stats()
        if k >= 1:
            # every block that finish k-1 pooled has been taken: the same shape asks for at least the same sizes again
            assert alive["held_blocks"] == 0 and alive["held_bytes"] == 0, (shape, k, alive)
        assert alive["live_bytes"] > alive["held_bytes"]
        del sv
        st = pc.nothing_lost("%s cycle %d" % (shape, k))          # invariant 1 after every cycle
        after.append(st)
        per_cycle.append(_delta(before, st))
        print(shape, "cycle", k, st, per_cycle[-1])
    cap = 1024 * pc.MiB
    assert 0 < after[0]["held_bytes"] < cap                      # (below the cap: nothing was evicted, the relations below are exact)
    assert per_cycle[0]["hits"] == 0 and per_cycle[0]["misses"] > 0
    for k in range(1, 5):
        assert after[k]["live_bytes"] == after[0]["live_bytes"], (shape, k, after)
        assert after[k]["held_bytes"] == after[0]["held_bytes"] and after[k]["held_blocks"] == after[0]["held_blocks"], (shape, k, after)
        assert per_cycle[k]["hits"] >= after[k - 1]["held_blocks"] > 0, (shape, k, per_cycle, after)
        assert per_cycle[k]["misses"] < per_cycle[0]["misses"], (shape, k, per_cycle)
        # the same shape makes the same requests: those the pool served are exactly the ones the driver no longer sees
        assert per_cycle[k]["hits"] + per_cycle[k]["misses"] == per_cycle[0]["misses"], (shape, k, per_cycle)
    pc.trim()
    st = pc.stats()
    assert st["live_bytes"] == 0 and st["held_bytes"] == 0, st


# ---------------------------------------------------------------- 3: batches
def _batch_rounds(run, tag):
    after = []
    for r in range(2):
        before = pc.stats()
        run("A")
        st = pc.nothing_lost("%s round %d" % (tag, r))
        after.append((st, _delta(before, st)))
        print(tag, "round", r, after[-1])
    assert after[1][0]["live_bytes"] == after[0][0]["live_bytes"], (tag, after)
    assert after[1][1]["hits"] > 0 and after[0][1]["hits"] == 0, (tag, after)
    assert after[1][1]["misses"] < after[0][1]["misses"], (tag, after)


@pytest.mark.parametrize("linear_solver", ["hip_indirect", "hip_dense"])
def test_batch_of_64_config5_members_recycles(linear_solver):
    run = pc.config5_group(64, linear_solver, max_iters=10)
    _batch_rounds(run, "config5 x 64 " + linear_solver)


def test_grouped_batch_with_spectral_and_complex_psd_members_recycles():
    import test_group_cones_gpu as tg
    run = pc.group_family(tg.MIX, "qp", 16, dict(max_iters=100))
    _batch_rounds(run, "spectral + complex PSD group")


# ---------------------------------------------------------------- 4: the cap (one child process each)
def _child(code, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    head = ("import sys\nfor p in (%r, %r, %r):\n    sys.path.insert(0, p)\n" % (ROOT, os.path.join(ROOT, "scs-python_amd"), os.path.join(ROOT, "tests")))
    p = subprocess.run([sys.executable, "-c", head + code], env=e, capture_output=True, text=True, timeout=timeout)
    print(p.stdout[-6000:])
    assert p.returncode == 0, "child exit status %d\n%s\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    return p.stdout


_CAP_ZERO = r'''
import gc
import scs
import pool_cases as pc
shapes = [(pc.generated("config5", "A"), dict(linear_solver="hip_dense", max_iters=10)),
          (pc.generated("lp_soc_big", "A"), dict(max_iters=10)),
          ((pc.feasible_qp(pc.KITCHEN, 3), pc.KITCHEN), dict(max_iters=30))]
pc.trim()
for (data, cone), stg in shapes:
    for k in range(3):
        sv = scs.SCS(data, cone, verbose=False, **stg)
        sv.solve()
        st = pc.stats()
        assert st["held_bytes"] == 0 and st["held_blocks"] == 0 and st["live_bytes"] > 0, st
        del sv
        gc.collect()
        st = pc.stats()
        assert st["held_bytes"] == 0 and st["held_blocks"] == 0 and st["live_bytes"] == 0, st
assert pc.stats()["hits"] == 0
print("CAP0 OK", pc.stats())
'''


def test_cap_zero_pools_nothing():
    assert "CAP0 OK" in _child(_CAP_ZERO, {"SCS_HIP_POOL_MB": "0"})


_CAP_SHAPES = r'''
import gc
import scs
import pool_cases as pc
# X and Y: dense workspaces of different orders (G^-1 of 15.9 MB at n = 1350, 10.6 MB at n = 1100)
K = {"l": 1500, "q": [50] * 10}
X = (pc.generated("config5", "A"), dict(linear_solver="hip_dense", max_iters=10))
Y = ((pc.pg.gen_feasible(K, 1100, 30, 9, pc._proj_dual)[0], K), dict(linear_solver="hip_dense", max_iters=10))
'''

_CAP_MEASURE = _CAP_SHAPES + r'''
out = []
for (data, cone), stg in (X, Y):
    pc.trim()
    sv = scs.SCS(data, cone, verbose=False, **stg)
    sv.solve()
    del sv
    out.append(pc.nothing_lost()["held_bytes"])
print("POOLED", out[0], out[1])
'''

_CAP_SMALL = _CAP_SHAPES + r'''
CAP = CAP_MB << 20
reads = []
def read(tag):
    st = pc.stats()
    reads.append(st)
    assert st["held_bytes"] <= CAP, (tag, st)
    return st
def cycle(shape, tag):
    (data, cone), stg = shape
    sv = scs.SCS(data, cone, verbose=False, **stg)
    sv.solve()
    alive = read(tag + " alive")
    del sv
    gc.collect()
    st = read(tag + " finished")
    assert st["live_bytes"] == st["held_bytes"], (tag, st)      # invariant 1
    return alive, st
# each of X and Y fits under the cap, the two together do not
pc.trim()
_, sy = cycle(Y, "Y alone")
sy_bytes, sy_blocks = sy["held_bytes"], sy["held_blocks"]
pc.trim()
_, sx = cycle(X, "X alone")
sx_bytes = sx["held_bytes"]
assert 0 < sy_bytes <= CAP and 0 < sx_bytes <= CAP and sx_bytes + sy_bytes > CAP, (sx_bytes, sy_bytes, CAP)
# the pool now holds X's blocks; Y's do not fit next to them: the OLDEST (X's) leave, Y's stay — all of them
before = pc.stats()
alive, after = cycle(Y, "Y after X")
assert after["held_bytes"] <= CAP and after["held_bytes"] >= sy_bytes, (after, sy_bytes)
assert after["held_bytes"] - sy_bytes < sx_bytes                   # (part of X was returned to the driver)
# ... which a second Y shows: it finds every block of its own (as many hits as Y pooled), the pool keeps only X's remainder
h0 = pc.stats()
(data, cone), stg = Y
sv = scs.SCS(data, cone, verbose=False, **stg)
sv.solve()
st = read("second Y alive")
assert st["hits"] - h0["hits"] >= sy_blocks, (st, h0, sy_blocks)
assert st["held_bytes"] == after["held_bytes"] - sy_bytes, (st, after, sy_bytes)
del sv
gc.collect()
st = read("second Y finished")
assert st["live_bytes"] == st["held_bytes"], st
for k in range(3):                                                 # alternating shapes never exceed the cap and lose nothing
    cycle(X, "X %d" % k)
    cycle(Y, "Y %d" % k)
pc.trim()
st = pc.stats()
assert st["live_bytes"] == 0 and st["held_bytes"] == 0, st
print("CAPSMALL OK", len(reads), "reads; pooled bytes X", sx_bytes, "Y", sy_bytes, "cap", CAP)
'''


def test_cap_smaller_than_two_workspaces_evicts_the_oldest_blocks():
    # the cap is chosen from what the two workspaces pool under the default cap (measured in a child of its own): the larger of
    # the two rounded up to the next MiB, plus one
    line = [ln for ln in _child(_CAP_MEASURE).splitlines() if ln.startswith("POOLED")][-1]
    sx, sy = (int(v) for v in line.split()[1:])
    cap_mb = -(-max(sx, sy) // pc.MiB) + 1
    assert sx + sy > cap_mb * pc.MiB, (sx, sy, cap_mb)
    assert "CAPSMALL OK" in _child("CAP_MB = %d\n" % cap_mb + _CAP_SMALL, {"SCS_HIP_POOL_MB": str(cap_mb)})


# ---------------------------------------------------------------- 5: refused and failed setups
def test_refused_setups_lose_nothing():
    import scs
    import spectral_ref as sr
    # a workspace that exists, so that the pool is not trivially empty
    (data, cone), stg = _cycle_shapes()["config5_arena"]()
    sv = scs.SCS(data, cone, verbose=False, **stg)
    sv.solve()
    del sv
    base = pc.nothing_lost("base")
    for bad, why in (({"d": [65]}, "exceeds the supported order 64"), ({"nuc_m": [8193], "nuc_n": [1]}, "m n exceeds 8192"),
                     ({"sl_n": [4], "sl_k": [5]}, "1 <= k <= n")):
        m = sr.m_of(bad)
        with pytest.raises(ValueError, match="ScsWork allocation error") as e:
            scs.SCS(dict(A=sp.eye(m, format="csc"), b=np.ones(m), c=np.ones(m)), bad, verbose=False)
        assert why in str(e.value)
        del e
        pc.nothing_lost(str(bad))
    with pytest.raises(ValueError, match="cone dimensions do not match m"):      # a bad cone: one row short
        scs.SCS(dict(A=sp.eye(5, format="csc"), b=np.ones(5), c=np.ones(5)), {"l": 2, "q": [4]}, verbose=False)
    pc.nothing_lost("bad cone")
    n = 8193                                                                       # HIP_DENSE beyond its largest order
    big = dict(A=sp.eye(n, format="csc"), b=np.ones(n), c=np.ones(n))
    with pytest.raises(ValueError, match="hip_dense: n = 8193 exceeds 8192") as e:
        scs.SCS(big, {"l": n}, linear_solver=scs.LinearSolver.HIP_DENSE, verbose=False)
    del e
    st = pc.nothing_lost("dense beyond 8192")
    assert st["live_bytes"] >= 0 and st["held_bytes"] <= 1024 * pc.MiB
    print("refused setups:", base, "->", st)


# ---------------------------------------------------------------- 6: threads
def test_eight_threads_cycling_their_own_shapes():
    import scs
    import problem_gen as pg
    shapes = []
    for t in range(8):
        K = {"l": 300 + 40 * t, "q": [10] * (10 + t)}
        shapes.append((pg.gen_feasible(K, 200 + 30 * t, 10, 60 + t, pc._proj_dual)[0], K))
    pc.trim()
    last, errors = [None] * 8, []

    def work(t):
        try:
            data, K = shapes[t]
            for _ in range(4):
                sv = scs.SCS(data, K, verbose=False, linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=400)
                last[t] = sv.solve(warm_start=False)
                del sv
                gc.collect()
        except BaseException as e:  # noqa: BLE001 (reported below, in the main thread)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=240)
    assert not any(th.is_alive() for th in threads)
    assert not errors, errors
    st = pc.nothing_lost("after the join")
    assert st["hits"] > 0
    for t, (data, K) in enumerate(shapes):
        solo = scs.SCS(data, K, verbose=False, linear_solver=scs.LinearSolver.HIP_INDIRECT, max_iters=400).solve(warm_start=False)
        pc.same_bits(last[t], solo, "thread %d" % t)
    pc.nothing_lost("after the solo solves")


# ---------------------------------------------------------------- 7: recycled memory does not change results
def _family_names():
    return ["lp_soc", "exp_power_box", "psd", "complex_psd", "hip_dense", "aa_type1", "aa_type2", "aa_off", "warm_start",
            "warm_start_dense", "kitchen_solo", "group_config5_indirect", "group_config5_dense", "spectral_logdet", "spectral_nuclear",
            "spectral_ell1", "spectral_sum_largest", "group_ell1_short", "group_ell1_long", "group_sl", "group_d", "group_d64",
            "group_nuc_small", "group_nuc_largest", "group_soc_long", "group_cs_mix", "group_mix"]


def test_family_list_is_complete():
    assert sorted(_family_names()) == sorted(pc.families())


@pytest.mark.parametrize("family", _family_names())
def test_a_b_a_on_recycled_blocks_is_bit_identical(family):
    """A on driver-fresh blocks, B (same shape, other data, seed and scale) on A's blocks, A again on B's: the third solve returns the
    bits of the first.  hits > 0 in the third: it did run on recycled blocks."""
    run = pc.families()[family]
    pc.trim()
    s0 = pc.stats()
    first = run("A")
    s1 = pc.nothing_lost(family + " first A")
    assert s1["hits"] == s0["hits"], "the first solve was meant to run on fresh blocks"
    run("B")
    s2 = pc.nothing_lost(family + " B")
    third = run("A")
    s3 = pc.nothing_lost(family + " second A")
    print(family, "hits in B", s2["hits"] - s1["hits"], "hits in the second A", s3["hits"] - s2["hits"], "held", s3["held_bytes"])
    assert s2["hits"] > s1["hits"] and s3["hits"] > s2["hits"], (s1, s2, s3)
    assert s3["live_bytes"] == s1["live_bytes"], (s1, s3)
    assert len(first) == len(third) > 0
    for i, (a, b) in enumerate(zip(first, third)):
        pc.same_bits(a, b, "%s result %d" % (family, i))
        assert a["info"]["status_val"] != -4, a["info"]       # (never "failed": the iterates are finite)


# ---------------------------------------------------------------- 8: the same under poison (labs build)
_POISON = r'''
import numpy as np
import pool_cases as pc
from scs import _scs_hip
assert _scs_hip.labs_build()
fam = pc.families()
for name in NAMES:
    run = fam[name]
    pc.trim()
    s0 = pc.stats()
    first = run("A")
    s1 = pc.nothing_lost(name)
    assert s1["hits"] == s0["hits"], (name, "first cycle not on fresh blocks")
    second = run("A")
    s2 = pc.nothing_lost(name)
    assert s2["hits"] > s1["hits"], (name, s1, s2)
    for i, (a, b) in enumerate(zip(first, second)):
        for key in ("x", "y", "s"):
            assert np.isfinite(b[key]).all(), (name, i, key, "non-finite on poisoned blocks")
        pc.same_bits(a, b, "%s result %d (poisoned blocks)" % (name, i))
    print("POISON OK", name, "hits", s2["hits"] - s1["hits"], flush=True)
print("POISON ALL OK", len(NAMES))
'''


@pytest.mark.labs
def test_recycled_blocks_filled_with_0xff_do_not_change_results():
    """SCS_HIP_POOL_POISON=1 (labs build): every recycled block arrives filled with 0xFF bytes (NaN as a double, -1 as an int).  The
    second cycle of every family runs on such blocks and returns the bits of the first, which ran on fresh ones; no NaN appears."""
    names = _family_names()
    out = _child("NAMES = %r\n" % (names,) + _POISON, {"SCS_HIP_POOL_POISON": "1"}, timeout=900)
    assert "POISON ALL OK %d" % len(names) in out
    for n in names:
        assert "POISON OK %s " % n in out
