"""Dense GARE timing: ms per solve(GAREProblem, MatrixSign()) on SteelProfile(n) (G = B B', Q = C'C), sign iterations, Newton-Kleinman
refinements and the scaled residuals, and the split from the library's own kernel timers: the Gauss-Jordan inversions (all gj_* classes,
the refinement's SignLyap included), the K W K GEMMs of the sign iteration, the update kernel, the QR extraction, the residual GEMMs and
the refinement's sign/replay GEMMs.  For the kernel split as the hardware sees it run this under
`rocprofv3 --kernel-trace --stats -d <dir> -o gare -- python tools/time_dense_gare.py`.
  python tools/time_dense_gare.py [--reps R] [--panel auto|register|tournament] [n ...]      (default n: 371 1357 5177)"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

PANEL = {"auto": 0, "register": 1, "tournament": 2}
ap = argparse.ArgumentParser()
ap.add_argument("--panel", choices=sorted(PANEL), default="auto")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
ctx = D.default_context()
ctx.set_option("dense_gj_panel", PANEL[args.panel])
for n in args.n or [371, 1357, 5177]:
    d = D.steel_profile(n)
    are = D.GAREProblem(d.E, d.A, D.lowrank(d.B), D.lowrank(np.ascontiguousarray(d.C.T)))
    D.solve(are, D.MatrixSign())                                  # warm-up (pool, code objects)
    times = []
    for _ in range(max(1, args.reps)):
        t = time.perf_counter()
        X, info = D.solve(are, D.MatrixSign(), return_info=True)
        times.append(time.perf_counter() - t)
    ctx.prof_enable(True); ctx.prof_reset()                       # a separate run under the library's kernel timers (they cost wall time)
    D.solve(are, D.MatrixSign())
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    ms = lambda pred: sum(v["ms"] for k, v in prof.items() if pred(k))
    tot = ms(lambda k: True)
    parts = dict(inversions=ms(lambda k: k.startswith("gj_")), kwk_gemms=ms(lambda k: k == "are_kwk"), update=ms(lambda k: k == "are_update"),
                 qr_extraction=ms(lambda k: k in ("qr_panel", "gemm_qr", "gemm_qr_wide_tn", "gemm_qr_wide_nn", "are_extract", "are_extract_ops")),
                 residual=ms(lambda k: k.startswith("are_residual")), refinement_gemms=ms(lambda k: k == "sign_gemm"))
    split = ", ".join(f"{k} {100 * v / max(tot, 1e-9):.0f} %" for k, v in parts.items())
    print(f"n={n} panel={args.panel}: {1e3 * min(times):.1f} ms per solve (best of {len(times)}; median {1e3 * float(np.median(times)):.1f}); "
          f"{info['iters']} sign iterations, {info['refinements']} refinements, scaled residual {info['res0']:.2e} -> {info['res']:.2e}; "
          f"timed kernels {tot:.1f} ms: {split}", flush=True)
