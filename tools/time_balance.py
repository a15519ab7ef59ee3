"""Device SVD and balanced truncation timing.

Part 1: `dre_svd_jacobi` (operand resident on the device) against `dre_host_svd_left` (the scalar one-sided Jacobi on the host that the
Projection strategy uses) and `numpy.linalg.svd`, alternated over `--rounds` rounds after a warm-up round in ONE process.  Inputs: the matrices
Z_o'E Z_c of steel_profile(n, convection=3e-3) for every `--n` (default 371 and 1357; formed on the host from the device's factored Gramians)
and random 224 x 224 and 512 x 512.  With sweeps and rounds per call and, under the library's kernel timers, the per-launch time of the round
kernel.
Part 2: the breakdown of one `balanced_truncation` into factorisation, two replays, SVD + projection (`dre_balance_lr`), and `dre_balance_lr`'s
own split per kernel tag.
  python tools/time_balance.py [--rounds 3] [--n 371 1357] [--no-random]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D
from dre_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--n", type=int, nargs="*", default=[371, 1357])
ap.add_argument("--no-random", action="store_true")
args = ap.parse_args()
ctx = D.default_context()
fmt = lambda v: "/".join(f"{x:.2f}" for x in v)


def timed(f):
    ctx.sync()
    t = time.perf_counter()
    out = f()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t), out


def gramian_factors(d):
    """(sign, Ed, Ad, Bd, Cd, (Lc, Dc, Lo, Do) on the device, times of the factorisation and the two replays in ms)"""
    E, A, B, Cm = d.E.toarray(), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    Ed, Ad, Bd, Cd = (ctx.upload(M) for M in (E, A, B, Cm))
    Ctd, Iq, Im = ctx.upload(np.asfortranarray(Cm.T)), ctx.upload(np.eye(Cm.shape[0])), ctx.upload(np.eye(B.shape[1]))
    t_fac, sign = timed(lambda: D.SignFactorization(Ed, Ad, ctx=ctx))
    t_o, (Lo, Do, _) = timed(lambda: sign.solve_lr(Ctd, Iq, None, 256, 1, download=False))
    t_c, (Lc, Dc, _) = timed(lambda: sign.solve_lr(Bd, Im, None, 256, 1, download=False, transposed=True))
    sign.close()
    return (E, A, B, Cm), (Ed, Ad, Bd, Cd), (Lc, Dc, Lo, Do), (t_fac, t_o, t_c)


def hankel_matrix(E, fac):
    Lc, Dc, Lo, Do = (M.numpy() for M in fac)
    Z = []
    for L, Dm in ((Lc, Dc), (Lo, Do)):
        dd = np.diag(Dm)
        Z.append(L[:, dd > 0] * np.sqrt(dd[dd > 0]))
    return Z[1].T @ (E @ Z[0])


def device_svd(Md):
    up, sp, vp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ii = (C.c_int64 * 3)()
    ms, _ = timed(lambda: ctx.chk(ctx.lib.dre_svd_jacobi(ctx.ptr, Md.ptr, 0.0, C.byref(up), C.byref(sp), C.byref(vp), ii)))
    out = [dev.DenseMatrix(ctx, p) for p in (up, sp, vp)]
    return ms, out, tuple(int(x) for x in ii)


def host_jacobi(M):
    p, w = M.shape
    Mf, U, sv = np.asfortranarray(M), np.zeros((p, p), order="F"), np.zeros(p)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    t = time.perf_counter()
    rc = ctx.lib.dre_host_svd_left(p, w, ptr(Mf), ptr(U), ptr(sv))
    assert rc == 0
    return 1e3 * (time.perf_counter() - t), np.sort(sv)[::-1]


systems = {}
inputs = []
for n in args.n:
    d = D.steel_profile(n, convection=3e-3)
    systems[n] = gramian_factors(d)
    M = hankel_matrix(systems[n][0][0], systems[n][2])
    if M.shape[0] > M.shape[1]:
        M = M.T                       # (the host routine wants the short side first)
    inputs.append((f"Z_o'E Z_c of steel_profile({n}) ({M.shape[0]} x {M.shape[1]})", M))
if not args.no_random:
    for q in (224, 512):
        inputs.append((f"random {q} x {q}", np.random.default_rng(q).standard_normal((q, q))))

print("== SVD: device block Jacobi / host scalar Jacobi / numpy.linalg.svd, ms per call ==", flush=True)
for name, M in inputs:
    Md = ctx.upload(M)
    t = {"dev": [], "host": [], "numpy": []}
    for rnd in range(args.rounds + 1):                    # round 0 warms up
        a, (U, S, V), st = device_svd(Md)
        b, sv_host = host_jacobi(M)
        t0 = time.perf_counter()
        s_ref = np.linalg.svd(M, compute_uv=True)[1]
        c = 1e3 * (time.perf_counter() - t0)
        if rnd:
            t["dev"].append(a); t["host"].append(b); t["numpy"].append(c)
    U, s, V = U.numpy(), S.numpy().ravel(), V.numpy()
    res = np.linalg.norm(M - (U * s) @ V.T) / np.linalg.norm(M)
    ctx.prof_enable(True); ctx.prof_reset()
    device_svd(Md)
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    rk = prof.get("svj_round", dict(ms=0.0, launches=1))
    print(f"{name}: device {fmt(t['dev'])} (best {min(t['dev']):.2f}; {st[0]} sweeps, {st[1]} rounds, rank {st[2]}, residual {res:.1e}, "
          f"max |s - s_numpy| / s_1 {np.abs(s - s_ref).max() / s_ref[0]:.1e}), host Jacobi {fmt(t['host'])} (best {min(t['host']):.2f}; "
          f"max |s - s_numpy| / s_1 {np.abs(sv_host[:len(s_ref)] - s_ref).max() / s_ref[0]:.1e}), numpy {fmt(t['numpy'])} (best {min(t['numpy']):.2f})", flush=True)
    print(f"    round kernel: {rk['ms']:.2f} ms in {rk['launches']} launches = {1e3 * rk['ms'] / max(rk['launches'], 1):.1f} us per launch; "
          + ", ".join(f"{k} {v['ms']:.2f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:5]), flush=True)

print("== balanced_truncation, order chosen by tol = 1e-8: ms per part ==", flush=True)
for n in args.n:
    d = D.steel_profile(n, convection=3e-3)
    rows = []
    for rnd in range(args.rounds + 1):
        _, (Ed, Ad, Bd, Cd), fac, (t_fac, t_o, t_c) = gramian_factors(d)
        out = [C.c_void_p() for _ in range(6)]
        ii, dd = (C.c_int64 * 6)(), (C.c_double * 3)()
        if rnd == args.rounds:
            ctx.prof_enable(True); ctx.prof_reset()
        t_bal, _ = timed(lambda: ctx.chk(ctx.lib.dre_balance_lr(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, Cd.ptr, *(M.ptr for M in fac), 0, 1e-8,
                                                                  *(C.byref(p) for p in out), ii, dd)))
        keep = [dev.DenseMatrix(ctx, p) for p in out]
        if rnd:
            rows.append((t_fac, t_o, t_c, t_bal))
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    best = [min(r[i] for r in rows) for i in range(4)]
    print(f"n={n}: factorisation {best[0]:.2f}, observability replay {best[1]:.2f}, controllability replay {best[2]:.2f}, dre_balance_lr {best[3]:.2f} "
          f"(order {ii[0]}, rank {ii[1]}, r_c {ii[2]}, r_o {ii[3]}, {ii[5]} SVD sweeps, ||W'ET - I|| {dd[0]:.1e}); the sign factorisation is "
          f"{100 * best[0] / sum(best):.0f} % of the call", flush=True)
    print("    dre_balance_lr by tag: " + ", ".join(f"{k} {v['ms']:.2f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:6]), flush=True)
