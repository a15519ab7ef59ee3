"""Dense path timing: ms per time step of Ros1 / Ros2(MatrixSign()) on SteelProfile(371) (45 steps of dt = -100) and SteelProfile(1357)
(10 steps of dt = -100), sign iterations per Lyapunov solve, and the Gauss-Jordan inversion's rate from the library's own kernel timers
(panel kernel + interchanges vs the rank-nb update GEMMs).  For the kernel split as the hardware sees it run this under
`rocprofv3 --kernel-trace --stats -d <dir> -o dense -- python tools/time_dense.py`.
  python tools/time_dense.py [n ...]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

STEPS = {371: 45, 1357: 10}
ctx = D.default_context()
for n in [int(a) for a in sys.argv[1:]] or [371, 1357]:
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    X0 = D.lowrank(L, Dm).dense()
    nsteps = STEPS.get(n, 10)
    for Ros in (D.Ros1, D.Ros2):
        prob = D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4500.0 - 100.0 * nsteps))
        D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4400.0)), Ros(D.MatrixSign()), dt=-100.0)     # warm-up (pool, code objects)
        t = time.perf_counter()
        sol, st = D.solve(prob, Ros(D.MatrixSign()), dt=-100.0, return_stats=True)
        el = time.perf_counter() - t
        ctx.prof_enable(True); ctx.prof_reset()                  # a second run under the library's kernel timers (they cost wall time)
        D.solve(prob, Ros(D.MatrixSign()), dt=-100.0)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        its = [s["iters"] for s in st["solves"]]
        refs = sum(s["refinements"] for s in st["solves"])
        ms = lambda keys: sum(v["ms"] for k, v in prof.items() if k in keys)
        cnt = lambda key: prof.get(key, {}).get("launches", 0)
        t_panel, t_upd, t_unp = ms({"gj_panel"}), ms({"gj_update"}), ms({"gj_unpivot"})
        n_inv = cnt("gj_unpivot")
        t_inv = t_panel + t_upd + t_unp
        tf = 2.0 * n ** 3 * n_inv / (t_inv * 1e-3) / 1e12 if t_inv > 0 else float("nan")
        print(f"n={n} {Ros.__name__}(MatrixSign()): {nsteps} steps in {el:.3f} s = {1e3 * el / nsteps:.1f} ms/step; "
              f"sign iterations per factored pencil {its[::2 if Ros is D.Ros2 else 1]}, refinements {refs}; "
              f"{n_inv} inversions, {t_inv / max(n_inv, 1):.2f} ms each ({tf:.1f} TFLOP/s at 2n^3): panel {100 * t_panel / max(t_inv, 1e-9):.0f} %, "
              f"update GEMMs {100 * t_upd / max(t_inv, 1e-9):.0f} %, unpivot {100 * t_unp / max(t_inv, 1e-9):.0f} %; "
              f"sign/replay GEMMs {ms({'sign_gemm'}):.1f} ms, driver GEMMs {ms({'dense_ros'}):.1f} ms", flush=True)
