"""LQG balanced truncation timing, operands resident on the device.

Part 1: both Riccati solutions,
  (a) one `dre_dense_gare_solve_pair` (one Hamiltonian sign iteration, two extractions);
  (b) two `dre_dense_gare_solve`: the regulator on (E, A, B, C') and the filter as the regulator of the transposed problem (E', A', C', B),
      each with a sign iteration of its own.
Alternated over `--rounds` rounds after a warm-up round in ONE process, ms each, then (a) / (b) by medians.  (b) is code that the pair call
does not change, so it is the baseline; the exit status is 1 when (a) is slower than (b).
Part 2: the split of one pair call and of one `dre_lqg_balance` under the library's kernel timers (a pass of its own: the timers cost wall
time), and the wall time of the two parts of `lqg_balanced_truncation`.
Systems: n = 371 is SteelProfile(371) with its five rightmost poles moved into the right half plane; every other n is the generated
nonsymmetric plant of tests/_lqg_model.py (two unstable poles, m = 4, q = 3, seed n).
  python tools/time_lqg.py [--rounds 3] [n ...]          (default 371 1024)"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import scipy.linalg as sla
import dre_amd as D
from dre_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("n", type=int, nargs="*")
args = ap.parse_args()
ctx = D.default_context()
fmt = lambda v: "/".join(f"{x:.2f}" for x in v)
med = lambda v: float(np.median(v))


def timed(f):
    ctx.sync()
    t = time.perf_counter()
    out = f()
    ctx.sync()
    return out, 1e3 * (time.perf_counter() - t)


def system(n):
    if n == 371:
        d = D.steel_profile(371)
        E, A = d.E.toarray(), d.A.toarray()
        lam = np.sort(sla.eigvals(A, E).real)[::-1]
        return E, A - 1.001 * lam[4] * E, np.asarray(d.B, float), np.asarray(d.C, float)
    rng = np.random.default_rng(n)
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    A0 = -np.diag(np.linspace(0.5, 20.0, n)) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    A0[0, 0], A0[1, 1] = 0.7, 0.3
    return E, E @ A0, rng.standard_normal((n, 4)), rng.standard_normal((3, n))


def single(Ed, Ad, Bd, Ctd):
    xp, ii, dd = C.c_void_p(), (C.c_int64 * 2)(), (C.c_double * 2)()
    ctx.chk(ctx.lib.dre_dense_gare_solve(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, None, Ctd.ptr, None, 50, 0.0, 2, C.byref(xp), ii, dd))
    return dev.DenseMatrix(ctx, xp), (int(ii[0]), int(ii[1]), float(dd[1]))


def pair(Ed, Ad, Bd, Ctd):
    xp, yp, ii, dd = C.c_void_p(), C.c_void_p(), (C.c_int64 * 4)(), (C.c_double * 4)()
    ctx.chk(ctx.lib.dre_dense_gare_solve_pair(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, None, Ctd.ptr, None, 50, 0.0, 2, C.byref(xp), C.byref(yp), ii, dd))
    return dev.DenseMatrix(ctx, xp), dev.DenseMatrix(ctx, yp), (int(ii[0]), int(ii[1]), int(ii[3]), float(dd[1]), float(dd[3]))


def lqg_balance(Ed, Ad, Bd, Cd, X, Y, order):
    out = [C.c_void_p() for _ in range(9)]
    ii, dd = (C.c_int64 * 6)(), (C.c_double * 3)()
    ctx.chk(ctx.lib.dre_lqg_balance(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, Cd.ptr, X.ptr, Y.ptr, order, 1e-8, *(C.byref(p) for p in out), ii, dd))
    keep = [dev.DenseMatrix(ctx, p) for p in out]
    return keep, (int(ii[1]), int(ii[2]), int(ii[3]), int(ii[5]), float(dd[0]))


def top_tags(f, k=8):
    ctx.prof_enable(True); ctx.prof_reset()
    f()
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    tot = sum(v["ms"] for v in prof.values())
    return f"{tot:.2f} ms in kernels: " + ", ".join(f"{t} {v['ms']:.2f} ms / {v['launches']}" for t, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:k])


slower = False
for n in args.n or [371, 1024]:
    E, A, B, Cm = system(n)
    Ed, Ad, Bd, Cd, Ctd, Etd, Atd = (ctx.upload(np.asfortranarray(M)) for M in (E, A, B, Cm, Cm.T, E.T, A.T))
    t_a, t_b, t_reg, t_fil, t_bal = [], [], [], [], []
    for rnd in range(args.rounds + 1):                               # round 0 warms up (pool, code objects)
        (X, Y, ip), a = timed(lambda: pair(Ed, Ad, Bd, Ctd))
        (_, i1), b1 = timed(lambda: single(Ed, Ad, Bd, Ctd))
        (Yt, i2), b2 = timed(lambda: single(Etd, Atd, Ctd, Bd))
        (_, ib), bal = timed(lambda: lqg_balance(Ed, Ad, Bd, Cd, X, Y, 16))
        if rnd:
            t_a.append(a); t_b.append(b1 + b2); t_reg.append(b1); t_fil.append(b2); t_bal.append(bal)
    dy = np.linalg.norm(Y.numpy() - Yt.numpy()) / np.linalg.norm(Yt.numpy())
    ratio = med(t_a) / med(t_b)
    slower |= ratio > 1.0
    print(f"n={n}: (a) pair {fmt(t_a)} ms ({ip[0]} iterations, refinements {ip[1]}/{ip[2]}, res {ip[3]:.1e}/{ip[4]:.1e}); (b) two single solves "
          f"{fmt(t_b)} ms = regulator {fmt(t_reg)} ({i1[0]} iterations) + transposed filter {fmt(t_fil)} ({i2[0]} iterations); (a) / (b) {ratio:.3f}; "
          f"|Y_pair - Y_single| / |Y| {dy:.1e}; dre_lqg_balance to order 16 {fmt(t_bal)} ms (rank {ib[0]}, r_c {ib[1]}, r_o {ib[2]}, {ib[3]} sweeps, "
          f"eye {ib[4]:.1e}); lqg_balanced_truncation = pair + balance {med(t_a) + med(t_bal):.2f} ms", flush=True)
    print("    one pair call:       " + top_tags(lambda: pair(Ed, Ad, Bd, Ctd)), flush=True)
    print("    one single call:     " + top_tags(lambda: single(Ed, Ad, Bd, Ctd)), flush=True)
    print("    one dre_lqg_balance: " + top_tags(lambda: lqg_balance(Ed, Ad, Bd, Cd, X, Y, 16)), flush=True)
sys.exit(1 if slower else 0)
