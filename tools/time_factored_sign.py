"""Factored sign solver timing on SteelProfile(n): ms for the sign factorisation (`dre_sign_create`), ms per factored replay (`solve_lr`) and
ms per dense replay (`MatrixSign`'s `solve()` on the same kept factorisation) for a Ros1-like right-hand side, operands resident on the
device, the two replays alternated over `--rounds` rounds after a warm-up round; then, in a separate pass under the library's kernel
timers, the split of `solve_lr` into thin GEMMs / QR / eigensolver / rest.  For the kernel table as the hardware sees it run this under
`rocprofv3 --kernel-trace --stats -d <dir> -o flr -- python tools/time_factored_sign.py`.
  python tools/time_factored_sign.py [--rounds 3] [--max-width 256] [--rtol r] [n ...]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--max-width", type=int, default=256)
ap.add_argument("--rtol", type=float, default=None)
ap.add_argument("--tau", type=float, default=100.0)
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
ctx = D.default_context()


def timed(f):
    ctx.sync()
    t = time.perf_counter()
    out = f()
    ctx.sync()
    return out, 1e3 * (time.perf_counter() - t)


for n in args.n or [371, 1357, 5177]:
    d = D.steel_profile(n)
    L0, D0 = D.initial_value(d)
    E, A, B, Cm = d.E.toarray(), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    tau, q = args.tau, Cm.shape[0]
    BtLD, EtL = (B.T @ L0) @ D0, E.T @ L0
    F = A - E / (2.0 * tau) - B @ (BtLD @ EtL.T)                     # the first Ros1 step's operator and right-hand side (lowrank_ros1.jl:39-44)
    G = np.hstack([Cm.T, EtL])
    S = np.zeros((G.shape[1],) * 2)
    S[:q, :q] = np.eye(q)
    S[q:, q:] = BtLD.T @ BtLD + D0 / tau
    Ed, Fd, Gd, Sd, Rd = (ctx.upload(M) for M in (E, F, G, S, G @ S @ G.T))
    D.SignFactorization(Ed, Fd, ctx=ctx).close()                     # warm-up (pool, code objects)
    sign, t_create = timed(lambda: D.SignFactorization(Ed, Fd, ctx=ctx))
    lr = lambda mr=1: sign.solve_lr(Gd, Sd, args.rtol, args.max_width, mr, download=False)
    dense = lambda: sign.solve_dense(Rd, download=False)
    t_lr, t_lr0, t_dn = [], [], []
    for rnd in range(args.rounds + 1):                               # round 0 warms up
        (_, _, info), a = timed(lr)
        (_, _, info0), a0 = timed(lambda: lr(0))
        (_, dinfo), b = timed(dense)
        if rnd:
            t_lr.append(a); t_lr0.append(a0); t_dn.append(b)
    ctx.prof_enable(True); ctx.prof_reset()                          # the split, in a pass of its own (the timers cost wall time)
    lr()
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    sign.close()
    ms = lambda pred: sum(v["ms"] for k, v in prof.items() if pred(k))
    total = ms(lambda k: True)
    thin = ms(lambda k: k == "signlr_gemm")
    qr = ms(lambda k: k.startswith("gemm_qr") or k.startswith("qr") or k.startswith("tsqr"))
    eig = ms(lambda k: k.startswith("sym_"))
    fmt = lambda v: "/".join(f"{x:.1f}" for x in v)
    print(f"n={n}: sign factorisation {t_create:.1f} ms ({sign.iters} iterations); solve_lr {fmt(t_lr)} ms (rank {info['rank']}, peak {info['peak_width']}, "
          f"{info['compressions']} compressions, {info['refinements']} refinements, res {info['res0']:.1e} -> {info['res']:.1e}); "
          f"solve_lr without refinement {fmt(t_lr0)} ms (res {info0['res']:.1e}); dense replay {fmt(t_dn)} ms ({dinfo['refinements']} refinements, "
          f"res {dinfo['res']:.1e}); kernel timers of one solve_lr: {total:.1f} ms = thin GEMMs {thin:.1f} + QR {qr:.1f} + eigensolver {eig:.1f} + rest "
          f"{total - thin - qr - eig:.1f}", flush=True)
    for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:8]:
        print(f"    {k:24s} {v['ms']:9.2f} ms  {v['launches']:6d} launches")
