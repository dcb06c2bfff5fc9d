"""One shared A, K = 256 config-5-shaped problems with their own feasible (b_i, c_i): what does sharing the matrix buy?

Three legs, each measured in fresh child processes that are started in turn (a, b, c, a, b, c, ...: drift of the box hits all alike):
  (a) independent   K full workspaces SCS(data), each update(b_i, c_i), one solve_batch     [--parent-root: a checkout of the parent commit]
  (b) shared        one workspace + K - 1 clones, update, solve_batch, tiled kernel OFF     [labs build, SCS_HIP_SHARED_TILE=0]
  (c) tiled         the same with the tiled CSR-stream kernel ON                             [labs build, SCS_HIP_SHARED_TILE=1]
All three run the same iterates (init, then update): the digest of every member's x, y, s must agree between the legs.

  python tools/shared_batch_bench.py --parent-root /path/to/parent/checkout [--labs-lib .../libscs_hip_labs.so] [--members 256] [--rounds 3]
  python tools/shared_batch_bench.py --leg shared --members 256 --repeats 3          (one leg, this checkout; prints one JSON line)

A child warms the process up with one small solve, then repeats [build K workspaces | solve_batch | tear down] `--repeats` times;
setup_s covers construction / cloning and the updates, solve_s the solve_batch call (deferred first setup included: it is part of
every leg's first solve).  The parent prints, per leg, the median over all children's repeats and the min-max spread."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    root = args.root or HERE
    sys.path[:0] = [root, os.path.join(root, "scs-python_amd")]
    import numpy as np
    import scs
    from scs import _scs_hip
    import problem_gen as pg

    def proj(z, K):
        return _scs_hip.proj_cone(z, K, dual=True)

    K, n, k, seed = pg.workload("config5_small")
    data, _, _ = pg.gen_feasible(K, n, k, seed, proj)
    A = data["A"]
    m = A.shape[0]
    rng = np.random.default_rng(2024)
    B, Cm = np.empty((args.members, m)), np.empty((args.members, n))
    for i in range(args.members):  # problem_gen's construction over the fixed A
        z = rng.standard_normal(m)
        y = np.asarray(proj(z, K), dtype=np.float64)
        B[i] = A @ rng.standard_normal(n) + (y - z)
        Cm[i] = -(A.T @ y)
    stg = dict(verbose=False, linear_solver=scs.LinearSolver.HIP_INDIRECT)
    scs.SCS(data, K, max_iters=50, **stg).solve()  # warm the process up (code objects, streams, pinned pool)
    tiled0 = _scs_hip.tiled_launches() if hasattr(_scs_hip, "tiled_launches") else 0
    reps = []
    digest = None
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        if args.leg == "independent":
            members = [scs.SCS(data, K, **stg) for _ in range(args.members)]
        else:
            parent = scs.SCS(data, K, **stg)
            members = [parent] + [parent.clone() for _ in range(args.members - 1)]
        for sv, b, c in zip(members, B, Cm):
            sv.update(b, c)
        t1 = time.perf_counter()
        res = scs.solve_batch(members)
        t2 = time.perf_counter()
        del members
        if args.leg != "independent":
            del parent
        iters = sum(r["info"]["iter"] for r in res)
        h = hashlib.sha256()
        for r in res:
            for key in ("x", "y", "s"):
                h.update(np.ascontiguousarray(r[key]).tobytes())
        digest = h.hexdigest()[:16]
        reps.append({"setup_s": t1 - t0, "solve_s": t2 - t1, "iters": iters, "solved": sum(r["info"]["status_val"] == 1 for r in res)})
    print(json.dumps({"leg": args.label or args.leg, "members": args.members, "reps": reps, "digest": digest,
                      "tiled_launches": (_scs_hip.tiled_launches() - tiled0) if hasattr(_scs_hip, "tiled_launches") else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["independent", "shared"])
    ap.add_argument("--label")
    ap.add_argument("--root")
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root")
    ap.add_argument("--labs-lib", default=os.path.join(HERE, "scs-python_amd", "scs", "libscs_hip_labs.so"))
    args = ap.parse_args()
    if args.leg:
        child(args)
        return
    if not args.parent_root:
        ap.error("--parent-root: leg (a) runs from a checkout of the parent commit (built there)")
    if not os.path.exists(args.labs_lib):
        ap.error("legs (b) and (c) need the labs build (%s): the switch of the tiled kernel is a labs switch" % args.labs_lib)
    base = [sys.executable, os.path.abspath(__file__), "--members", str(args.members), "--repeats", str(args.repeats)]
    legs = [
        ("a independent (parent)", base + ["--leg", "independent", "--root", args.parent_root], {}),
        ("b shared, per-member", base + ["--leg", "shared"], {"SCS_HIP_LIB": args.labs_lib, "SCS_HIP_SHARED_TILE": "0"}),
        ("c shared, tiled", base + ["--leg", "shared"], {"SCS_HIP_LIB": args.labs_lib, "SCS_HIP_SHARED_TILE": "1"}),
    ]
    out = {name: [] for name, _, _ in legs}
    digests = {}
    for rnd in range(args.rounds):
        for name, cmd, env in legs:
            e = dict(os.environ)
            e.pop("SCS_HIP_LIB", None)
            e.update(env)
            r = subprocess.run(cmd + ["--label", name], env=e, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit("leg %s failed:\n%s" % (name, r.stderr[-3000:]))
            rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            out[name].extend(rec["reps"])
            digests.setdefault(name, set()).add(rec["digest"])
            print("round %d  %-24s %s  tiled launches %s" % (rnd, name, "  ".join("%.3f+%.3f s" % (q["setup_s"], q["solve_s"]) for q in rec["reps"]),
                                                            rec["tiled_launches"]), flush=True)
    print("\n%d members, %d rounds x %d repeats per leg (median [min .. max])" % (args.members, args.rounds, args.repeats))
    print("%-24s %-28s %-28s %-30s %s" % ("leg", "setup s", "solve s", "ADMM iterations / s (solve)", "digest"))
    for name, _, _ in legs:
        reps = out[name]

        def fmt(vals, f):
            return (f + " [" + f + " .. " + f + "]") % (statistics.median(vals), min(vals), max(vals))

        print("%-24s %-28s %-28s %-30s %s" % (name, fmt([q["setup_s"] for q in reps], "%.3f"), fmt([q["solve_s"] for q in reps], "%.3f"),
                                             fmt([q["iters"] / q["solve_s"] for q in reps], "%.0f"), ",".join(sorted(digests[name]))))
    same = len(set().union(*digests.values())) == 1
    print("iterates equal across the legs: %s" % ("yes" if same else "NO"))


if __name__ == "__main__":
    main()
