"""Batched dense GARE timing: `solve_batch` with B GAREProblem members against B sequential `solve(GAREProblem, MatrixSign())` calls on
SteelProfile(n), members that differ in the input weight.  After a warm-up the two are alternated over --rounds rounds and the best of
each is reported as ms per member, with their ratio; then one batched run under the library's kernel timers gives the per-tag split
(`prof_stats()`).
  python tools/time_dense_gare_batch.py [--rounds 3] [--batches 1,4,16] [n ...]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

BATCHES = {371: (1, 4, 16), 1357: (1, 4)}
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", default="")
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
ctx = D.default_context()
alg = D.MatrixSign()
for n in args.n or [371, 1357]:
    d = D.steel_profile(n)
    E, A, Bm, Ct = d.E.toarray(), d.A.toarray(), np.asarray(d.B, dtype=float), np.ascontiguousarray(np.asarray(d.C, dtype=float).T)
    for B in ([int(b) for b in args.batches.split(",")] if args.batches else BATCHES.get(n, (1, 4))):
        probs = [D.GAREProblem(E, A, D.lowrank((1.0 + 0.05 * b) * Bm, np.eye(Bm.shape[1])), D.lowrank(Ct, np.eye(Ct.shape[1]))) for b in range(B)]
        out = D.solve_batch(probs, alg, return_stats=True)          # warm-up of both (pool, code objects)
        D.solve(probs[0], alg)
        tb, ts = [], []
        for _ in range(args.rounds):
            t = time.perf_counter(); D.solve_batch(probs, alg); tb.append(time.perf_counter() - t)
            t = time.perf_counter()
            for p in probs:
                D.solve(p, alg)
            ts.append(time.perf_counter() - t)
        per = lambda v: 1e3 * float(np.min(v)) / B
        ctx.prof_enable(True); ctx.prof_reset()
        D.solve_batch(probs, alg)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        tot = sum(v["ms"] for v in prof.values())
        split = ", ".join(f"{k} {v['ms']:.1f} ms ({100 * v['ms'] / max(tot, 1e-9):.0f} %)" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:8])
        its = [i["iters"] for _, i in out]
        print(f"n={n} B={B}: batched {per(tb):.2f} ms/member, sequential {per(ts):.2f} ms/member, ratio {per(ts) / per(tb):.2f} "
              f"(rounds batched {[round(1e3 * x, 1) for x in tb]} ms, sequential {[round(1e3 * x, 1) for x in ts]} ms; iters {its}); "
              f"kernel timers, {tot:.1f} ms: {split}", flush=True)
