"""Dense path timing: ms per time step of Ros1 / Ros2(MatrixSign()) on SteelProfile(n) (45 steps of dt = -100 at n = 371, 10 at 1357,
3 at 4096 and 5177), sign iterations per Lyapunov solve, and the Gauss-Jordan inversion's split from the library's own kernel timers:
the pivoting panel (register panel: panel kernel + interchanges; tournament panel: the selection rounds), the tournament's interchanges
and apply kernel, the rank-nb update GEMMs and the final unpivot.  For the kernel split as the hardware sees it run this under
`rocprofv3 --kernel-trace --stats -d <dir> -o dense -- python tools/time_dense.py`.
  python tools/time_dense.py [--panel auto|register|tournament] [--ros 1|2|12] [n ...]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

STEPS = {371: 45, 1357: 10, 4096: 3, 5177: 3}
PANEL = {"auto": 0, "register": 1, "tournament": 2}
ap = argparse.ArgumentParser()
ap.add_argument("--panel", choices=sorted(PANEL), default="auto")
ap.add_argument("--ros", default="12", help="1, 2 or 12 (both)")
ap.add_argument("--maxiters", type=int, default=40)
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
ctx = D.default_context()
ctx.set_option("dense_gj_panel", PANEL[args.panel])
MS = lambda: D.MatrixSign(maxiters=args.maxiters)
for n in args.n or [371, 1357]:
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    X0 = D.lowrank(L, Dm).dense()
    nsteps = STEPS.get(n, 3)
    for Ros in [R for R, c in ((D.Ros1, "1"), (D.Ros2, "2")) if c in args.ros]:
        prob = D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4500.0 - 100.0 * nsteps))
        D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4400.0)), Ros(MS()), dt=-100.0)     # warm-up (pool, code objects)
        t = time.perf_counter()
        sol, st = D.solve(prob, Ros(MS()), dt=-100.0, return_stats=True)
        el = time.perf_counter() - t
        ctx.prof_enable(True); ctx.prof_reset()                  # a second run under the library's kernel timers (they cost wall time)
        D.solve(prob, Ros(MS()), dt=-100.0)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        its = [s["iters"] for s in st["solves"]]
        refs = sum(s["refinements"] for s in st["solves"])
        ms = lambda keys: sum(v["ms"] for k, v in prof.items() if k in keys)
        cnt = lambda key: prof.get(key, {}).get("launches", 0)
        t_panel, t_swap, t_apply = ms({"gj_panel", "gj_tslu"}), ms({"gj_swap"}), ms({"gj_apply"})
        t_upd, t_unp = ms({"gj_update"}), ms({"gj_unpivot"})
        n_inv = cnt("gj_unpivot")
        t_inv = t_panel + t_swap + t_apply + t_upd + t_unp
        tf = 2.0 * n ** 3 * n_inv / (t_inv * 1e-3) / 1e12 if t_inv > 0 else float("nan")
        pc = lambda x: 100 * x / max(t_inv, 1e-9)
        print(f"n={n} panel={args.panel} {Ros.__name__}(MatrixSign()): {nsteps} steps in {el:.3f} s = {1e3 * el / nsteps:.1f} ms/step; "
              f"sign iterations per factored pencil {its[::2 if Ros is D.Ros2 else 1]}, refinements {refs}; "
              f"{n_inv} inversions, {t_inv / max(n_inv, 1):.2f} ms each ({tf:.1f} TFLOP/s at 2n^3): panel {pc(t_panel):.0f} %, "
              f"interchanges {pc(t_swap):.0f} %, apply {pc(t_apply):.0f} %, update GEMMs {pc(t_upd):.0f} %, unpivot {pc(t_unp):.0f} %; "
              f"sign/replay GEMMs {ms({'sign_gemm'}):.1f} ms, driver GEMMs {ms({'dense_ros'}):.1f} ms", flush=True)
