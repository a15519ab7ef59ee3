"""Adaptive dense Ros2 against the fixed grid on SteelProfile(n), tspan (4500, 0): fixed Ros2(MatrixSign()) at dt = -100 and the adaptive run
(first step -100, atol = 1e-3 rtol) at each rtol, interleaved, best of --reps.  Per run: accepted / rejected steps, ms per trial step (a
fixed step is a trial), sign iterations per trial, and the error of the final K against fixed Ros4(MatrixSign()) at dt = -10.  The last line
compares the adaptive runs' time per trial with the fixed step's (the added work per trial is two small launches and one read-back).
  python tools/time_dense_adaptive.py [--n 371] [--rtol 1e-2 1e-3 1e-4] [--reps 3]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=371)
ap.add_argument("--rtol", type=float, nargs="*", default=[1e-2, 1e-3, 1e-4])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-steps", type=int, default=20000)
args = ap.parse_args()
ctx = D.default_context()
MS = D.MatrixSign()
d = D.steel_profile(args.n)
L, Dm = D.initial_value(d)
X0 = D.lowrank(L, Dm).dense()
prob = D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 0.0))
D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4400.0)), D.Ros2(MS), dt=-100.0)       # warm-up (pool, code objects)
ref = D.solve(prob, D.Ros4(MS), dt=-10.0)
Kref = ref.K[-1]
runs = [("fixed dt=-100", None)] + [(f"adaptive rtol={r:g}", D.StepControl(rtol=r, atol=1e-3 * r, max_steps=args.max_steps)) for r in args.rtol]
best = {}
for rep in range(args.reps):
    for name, sc in runs:
        t = time.perf_counter()
        sol, st = D.solve(prob, D.Ros2(MS), dt=-100.0, adaptive=sc, return_stats=True)
        el = time.perf_counter() - t
        trials = st["lyapunov_solves"] // 2
        if name not in best or el < best[name][0]:
            best[name] = (el, trials, st.get("accepted", trials), st.get("rejected", 0), np.mean([s["iters"] for s in st["solves"][::2]]),
                          np.linalg.norm(sol.K[-1] - Kref) / np.linalg.norm(Kref))
for name, _ in runs:
    el, trials, acc, rej, its, err = best[name]
    print(f"n={args.n} {name}: accepted {acc} rejected {rej}; {el:.3f} s = {1e3 * el / trials:.2f} ms per trial step; "
          f"{its:.1f} sign iterations per trial; ||K(0) - K_ros4|| / ||K_ros4|| = {err:.3e}", flush=True)
fixed = best[runs[0][0]][0] / best[runs[0][0]][1]
print("ms per trial step, adaptive / fixed: " + ", ".join(f"{name.split()[1]} {best[name][0] / best[name][1] / fixed:.3f}" for name, _ in runs[1:]), flush=True)
