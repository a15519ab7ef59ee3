"""Batched block Jacobi timing: one `dre_svd_jacobi_batched` / `dre_sym_eig_jacobi_batched` call of B members against a loop of B single
calls (`dre_svd_jacobi` / `dre_sym_eig_jacobi`), operands resident on the device, alternated over `--rounds` rounds after a warm-up round in
ONE process.

SVD inputs: the Hankel matrices Z_o'E Z_c of steel_profile(n, convection=3e-3) for n = 371 and 1357 (93 x 110 and 116 x 134, formed as in
tools/time_balance.py from the device's factored Gramians); member b is that matrix with its rows and columns scaled by 1 + 1e-3 x (x standard
normal, seed b), so the members are different problems of one size, rank and grading.  Per member also `dre_host_svd_left`, the host Jacobi the Projection strategy uses.
Eigensolver inputs: the controllability Gramian of steel_profile(371) (order 371, numerically rank deficient) and its leading 202 x 202
block, scaled per member in the same way (symmetrically).
Then, under the library's kernel timers, the per-launch time of the batched round kernel at every B.
  python tools/time_jacobi_batch.py [--rounds 3] [--batches 1 4 16 32] [--n 371 1357]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D
from dre_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", type=int, nargs="*", default=[1, 4, 16, 32])
ap.add_argument("--n", type=int, nargs="*", default=[371, 1357])
args = ap.parse_args()
ctx = D.default_context()
lib = ctx.lib
fmt = lambda v: "/".join(f"{x:.2f}" for x in v)
harr = lambda hs: (C.c_void_p * len(hs))(*[h.ptr for h in hs])


def timed(f):
    ctx.sync()
    t = time.perf_counter()
    out = f()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t), out


def factors(n):
    """(E, Z_c, Z_o) of steel_profile(n, convection=3e-3) from the device's factored Gramians"""
    d = D.steel_profile(n, convection=3e-3)
    E, A, B, Cm = d.E.toarray(), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    Ed, Ad, Bd = (ctx.upload(M) for M in (E, A, B))
    Ctd, Iq, Im = ctx.upload(np.asfortranarray(Cm.T)), ctx.upload(np.eye(Cm.shape[0])), ctx.upload(np.eye(B.shape[1]))
    sign = D.SignFactorization(Ed, Ad, ctx=ctx)
    Lo, Do, _ = sign.solve_lr(Ctd, Iq, None, 256, 1)
    Lc, Dc, _ = sign.solve_lr(Bd, Im, None, 256, 1, transposed=True)
    sign.close()
    Z = []
    for L, Dm in ((Lc, Dc), (Lo, Do)):
        dd = np.diag(Dm)
        Z.append(L[:, dd > 0] * np.sqrt(dd[dd > 0]))
    return E, Z[0], Z[1]


def members(M, B, sym=False):
    """member b: diag(1 + 1e-3 x) M diag(1 + 1e-3 y) with x, y standard normal (seed b; y = x for a symmetric M): another problem of the same
    size, rank and grading"""
    out = []
    for b in range(B):
        rng = np.random.default_rng(b)
        x = 1.0 + 1e-3 * rng.standard_normal(M.shape[0])
        y = x if sym else 1.0 + 1e-3 * rng.standard_normal(M.shape[1])
        out.append(x[:, None] * M * y[None, :])
    return out


def free(handles):
    for p in handles:
        if p:
            lib.dre_dense_free(ctx.ptr, C.c_void_p(p))


def svd_single_loop(Ad):
    ii = (C.c_int64 * 3)()
    sweeps = []
    for A in Ad:
        u, s, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctx.chk(lib.dre_svd_jacobi(ctx.ptr, A.ptr, 0.0, C.byref(u), C.byref(s), C.byref(v), ii))
        free([u.value, s.value, v.value])
        sweeps.append(int(ii[0]))
    return sweeps


def svd_batched(Ad):
    nb = len(Ad)
    us, ss, vs = (C.c_void_p * nb)(), (C.c_void_p * nb)(), (C.c_void_p * nb)()
    ii, st = (C.c_int64 * (3 * nb))(), (C.c_int32 * nb)()
    ctx.chk(lib.dre_svd_jacobi_batched(ctx.ptr, nb, harr(Ad), 0.0, us, ss, vs, ii, st))
    assert not any(st)
    free(list(us) + list(ss) + list(vs))
    return [int(ii[3 * b]) for b in range(nb)]


def eig_single_loop(Ad):
    ii = (C.c_int64 * 2)()
    sweeps = []
    for A in Ad:
        w, v = C.c_void_p(), C.c_void_p()
        ctx.chk(lib.dre_sym_eig_jacobi(ctx.ptr, A.ptr, 0.0, C.byref(w), C.byref(v), ii))
        free([w.value, v.value])
        sweeps.append(int(ii[0]))
    return sweeps


def eig_batched(Ad):
    nb = len(Ad)
    ws, vs = (C.c_void_p * nb)(), (C.c_void_p * nb)()
    ii, st = (C.c_int64 * (2 * nb))(), (C.c_int32 * nb)()
    ctx.chk(lib.dre_sym_eig_jacobi_batched(ctx.ptr, nb, harr(Ad), 0.0, ws, vs, ii, st))
    assert not any(st)
    free(list(ws) + list(vs))
    return [int(ii[2 * b]) for b in range(nb)]


def host_jacobi(M):
    if M.shape[0] > M.shape[1]:
        M = M.T                       # (the host routine wants the short side first)
    p, w = M.shape
    Mf, U, sv = np.asfortranarray(M), np.zeros((p, p), order="F"), np.zeros(p)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    t = time.perf_counter()
    assert lib.dre_host_svd_left(p, w, ptr(Mf), ptr(U), ptr(sv)) == 0
    return 1e3 * (time.perf_counter() - t)


def compare(name, mats, single, batched, tag, host=None):
    for B in args.batches:
        Ad = [ctx.upload(M) for M in mats[:B]]
        t = {"loop": [], "batch": [], "host": []}
        for rnd in range(args.rounds + 1):                    # round 0 warms up
            a, sw_single = timed(lambda: single(Ad))
            b, sw_batch = timed(lambda: batched(Ad))
            c = sum(host(M) for M in mats[:B]) if host else 0.0
            assert sw_single == sw_batch
            if rnd:
                t["loop"].append(a); t["batch"].append(b); t["host"].append(c)
        ctx.prof_enable(True); ctx.prof_reset()
        batched(Ad)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        rk = prof.get(tag, dict(ms=0.0, launches=1))
        lb, bb = min(t["loop"]), min(t["batch"])
        line = (f"{name} B={B}: loop of single calls {fmt(t['loop'])} ms (best {lb:.2f}), batched {fmt(t['batch'])} ms (best {bb:.2f}) = "
                f"{lb / bb:.2f} x, {bb / B:.3f} ms per member; sweeps {min(sw_batch)} .. {max(sw_batch)}; {tag}: "
                f"{1e3 * rk['ms'] / max(rk['launches'], 1):.1f} us per launch in {rk['launches']} launches")
        if host:
            line += f"; host Jacobi {min(t['host']) / B:.3f} ms per member"
        print(line, flush=True)


print("== dre_svd_jacobi_batched against a loop of dre_svd_jacobi ==", flush=True)
gram = None
for n in args.n:
    E, Zc, Zo = factors(n)
    M = Zo.T @ (E @ Zc)
    if n == 371:
        gram = Zc @ Zc.T
    compare(f"Hankel matrix of steel_profile({n}) ({M.shape[0]} x {M.shape[1]})", members(M, max(args.batches)), svd_single_loop, svd_batched, "svjb_round",
            host=host_jacobi)
print("== dre_sym_eig_jacobi_batched against a loop of dre_sym_eig_jacobi ==", flush=True)
if gram is None:
    E, Zc, Zo = factors(371)
    gram = Zc @ Zc.T
for q in (202, 371):
    S = gram[:q, :q]
    compare(f"controllability Gramian of steel_profile(371), leading block of order {q}", members(0.5 * (S + S.T), max(args.batches), sym=True), eig_single_loop,
            eig_batched, "bjb_pivot")
