"""Batched dense path timing: `solve_batch` with B members against B sequential `solve` calls, Ros1(MatrixSign()), five steps of dt = -100
on SteelProfile(n), members that differ in the input weight.  After a warm-up the two are alternated over --rounds rounds and the median
of each is reported as ms per member-step, with their ratio; then one batched run under the library's kernel timers gives the per-tag
split (`prof_stats()`).
  python tools/time_dense_batch.py [--rounds 3] [--batches 1,4,16,64] [n ...]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

NSTEPS = 5
BATCHES = {371: (1, 4, 16, 64), 1357: (1, 4, 16)}
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", default="")
ap.add_argument("--maxiters", type=int, default=40)
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
ctx = D.default_context()
alg = lambda: D.Ros1(D.MatrixSign(maxiters=args.maxiters))
for n in args.n or [371, 1357]:
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    X0 = D.lowrank(L, Dm).dense()
    E, A = d.E.toarray(), d.A.toarray()
    tspan = (4500.0, 4500.0 - 100.0 * NSTEPS)
    for B in ([int(b) for b in args.batches.split(",")] if args.batches else BATCHES.get(n, (1, 4))):
        probs = [D.GDREProblem(E, A, (1.0 + 0.05 * b) * d.B, d.C, X0, tspan) for b in range(B)]
        D.solve_batch(probs, alg(), dt=-100.0)                      # warm-up of both (pool, code objects)
        D.solve(probs[0], alg(), dt=-100.0)
        tb, ts = [], []
        for _ in range(args.rounds):
            t = time.perf_counter(); D.solve_batch(probs, alg(), dt=-100.0); tb.append(time.perf_counter() - t)
            t = time.perf_counter()
            for p in probs:
                D.solve(p, alg(), dt=-100.0)
            ts.append(time.perf_counter() - t)
        per = lambda v: 1e3 * float(np.median(v)) / (B * NSTEPS)
        ctx.prof_enable(True); ctx.prof_reset()
        D.solve_batch(probs, alg(), dt=-100.0)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        tot = sum(v["ms"] for v in prof.values())
        split = ", ".join(f"{k} {v['ms']:.1f} ms ({100 * v['ms'] / max(tot, 1e-9):.0f} %)" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:8])
        print(f"n={n} B={B}: batched {per(tb):.2f} ms/member-step, sequential {per(ts):.2f} ms/member-step, ratio {per(ts) / per(tb):.2f} "
              f"(rounds batched {[round(1e3 * x, 1) for x in tb]} ms, sequential {[round(1e3 * x, 1) for x in ts]} ms); "
              f"kernel timers, {tot:.1f} ms: {split}", flush=True)
