"""Both Lyapunov equations of one pencil, timed on steel_profile(n, convection=3e-3), F = A - E / (2 tau), operands resident on the device:
  (a) one sign factorisation (`dre_sign_create`) + a primal dense replay (F'XE + E'XF = -C'C) + a dual dense replay (F Y E' + E Y F' = -B B')
      on the one handle;
  (b) the way without the dual replay: two factorisations, of (F, E) and of (F', E'), and one primal replay on each.
Three alternated rounds of (a), (b) after a warm-up round (`--rounds`), ms each, then the ratios dual replay / primal replay on the same handle
and (a) / (b), and the same ratio for single replays without refinement (`max_refine = 0`: the replays' own cost, whatever number of refinement
steps the two right-hand sides ask for); then one primal and one dual replay under the library's kernel timers (a pass of its own: the timers cost wall time).
  python tools/time_sign_pair.py [--rounds 3] [--tau 100] [n ...]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
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


fmt = lambda v: "/".join(f"{x:.2f}" for x in v)
med = lambda v: float(np.median(v))
for n in args.n or [371, 1357, 5177]:
    d = D.steel_profile(n, convection=3e-3)
    E, A, B, Cm = d.E.toarray(), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    F = A - E / (2.0 * args.tau)
    Ed, Fd, Etd, Ftd, Rod, Rcd = (ctx.upload(np.asfortranarray(M)) for M in (E, F, E.T, F.T, Cm.T @ Cm, B @ B.T))
    t_cr, t_pr, t_du, t_a, t_b, t_pr0, t_du0 = [], [], [], [], [], [], []
    for rnd in range(args.rounds + 1):                               # round 0 warms up (pool, code objects)
        sign, cr = timed(lambda: D.SignFactorization(Ed, Fd, ctx=ctx))
        (_, ip), pr = timed(lambda: sign.solve_dense(Rod, download=False))
        (_, idu), du = timed(lambda: sign.solve_dense(Rcd, download=False, transposed=True))
        _, pr0 = timed(lambda: sign.solve_dense(Rod, 0, download=False))
        _, du0 = timed(lambda: sign.solve_dense(Rcd, 0, download=False, transposed=True))
        sign.close()

        def two_factorisations():
            for Eh, Fh, Rh in ((Ed, Fd, Rod), (Etd, Ftd, Rcd)):
                s = D.SignFactorization(Eh, Fh, ctx=ctx)
                s.solve_dense(Rh, download=False)
                s.close()
        _, b = timed(two_factorisations)
        if rnd:
            t_cr.append(cr); t_pr.append(pr); t_du.append(du); t_a.append(cr + pr + du); t_b.append(b); t_pr0.append(pr0); t_du0.append(du0)
    print(f"n={n}: factorisation {fmt(t_cr)} ms ({sign.iters} iterations); primal replay {fmt(t_pr)} ms ({ip['refinements']} refinements, res {ip['res']:.1e}); "
          f"dual replay {fmt(t_du)} ms ({idu['refinements']} refinements, res {idu['res']:.1e}); dual / primal {med(t_du) / med(t_pr):.2f}; "
          f"without refinement: primal {fmt(t_pr0)} ms, dual {fmt(t_du0)} ms, dual / primal {med(t_du0) / med(t_pr0):.2f}; "
          f"(a) one factorisation + both replays {fmt(t_a)} ms; (b) two factorisations + a primal replay each {fmt(t_b)} ms; "
          f"(a) / (b) {med(t_a) / med(t_b):.2f}", flush=True)
    sign = D.SignFactorization(Ed, Fd, ctx=ctx)
    for name, tr, Rd in (("primal", False, Rod), ("dual", True, Rcd)):
        ctx.prof_enable(True); ctx.prof_reset()
        sign.solve_dense(Rd, download=False, transposed=tr)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        print(f"    kernel timers of one {name} replay: " + ", ".join(f"{k} {v['ms']:.2f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:5]), flush=True)
    sign.close()
