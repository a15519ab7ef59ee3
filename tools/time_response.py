"""Time-response timing: the step response and simulate (S = 1, 8) of one `dre_time_response` call with (a) the default block, (b) block = 1,
the per-step launch chain on the same code, and (c) the NumPy sequential recurrence x_{k+1} = M x_k + N w_k on the host (M and N by numpy.linalg.solve, once per order); with `--blocks` also
other powers of two.  Alternated over `--rounds` rounds after a warm-up round at each shape in ONE process, timed with a synchronised host
clock around the whole call (uploads of the operands excluded, the read-back of Y included).

Systems: steel_profile(371) and fixed-seed random stable pencils E = I + 0.1 N / sqrt(n), A = -(I + 0.4 N' / sqrt(n)) E at the other orders,
m = q = 4, dt = 0.01.  Then, under the library's kernel timers, the share of each kernel class in the default call.  `--only-default` runs
nothing but one warm-up and one default call per shape (for a kernel trace of its own).
  python tools/time_response.py [--rounds 3] [--n 371 1357 4096] [--K 1024 8192] [--S 1 8] [--blocks 16 256] [--chain-max 8192] [--host-max 128]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--n", type=int, nargs="*", default=[371, 1357, 4096])
ap.add_argument("--K", type=int, nargs="*", default=[1024, 8192])
ap.add_argument("--S", type=int, nargs="*", default=[1, 8])
ap.add_argument("--blocks", type=int, nargs="*", default=[])
ap.add_argument("--chain-max", type=int, default=8192, help="block = 1 runs at most this many steps; beyond it its whole time is scaled to K (which overstates it: the inversion is scaled too)")
ap.add_argument("--host-max", type=int, default=128, help="the host loop runs at most this many steps; its loop time is scaled to K")
ap.add_argument("--dt", type=float, default=0.01)
ap.add_argument("--only-default", action="store_true")
args = ap.parse_args()
ctx = D.default_context()
lib = ctx.lib
pd = C.POINTER(C.c_double)
fmt = lambda v: "/".join(f"{x:.1f}" for x in v)
M_, Q_ = 4, 4


def system(n):
    rng = np.random.default_rng(n)
    if n == 371:
        d = D.steel_profile(n)
        return d.E.toarray(), d.A.toarray(), rng.standard_normal((n, M_)), rng.standard_normal((Q_, n))
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    A = -(np.eye(n) + 0.4 * rng.standard_normal((n, n)) / np.sqrt(n)) @ E
    return E, A, rng.standard_normal((n, M_)), rng.standard_normal((Q_, n))


def call(ops, K, kind, U, block):
    """U: C-contiguous (S, K+1, m), made before the clock starts (a fresh host buffer per call would be pinned by the runtime inside the clock)"""
    S = U.shape[0] if kind == 2 else 0
    Y = np.zeros(S * (K + 1) * Q_ if kind == 2 else (K + 1) * Q_ * M_)
    info = (C.c_int64 * 4)()
    ctx.chk(lib.dre_time_response(ctx.ptr, *(o.ptr for o in ops), 0, args.dt, K, kind, U.ctypes.data_as(pd) if kind == 2 else None, S,
                                  None, block, Y.ctypes.data_as(pd), info))
    return Y, list(info)


def timed(f):
    ctx.sync()
    t = time.perf_counter()
    out = f()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t), out


def host_setup(E, A, B):
    P = E - 0.5 * args.dt * A
    return 2.0 * np.linalg.solve(P, E) - np.eye(E.shape[0]), 0.5 * args.dt * np.linalg.solve(P, B)


def host(Mx, N, Cm, K, kind, U):
    if kind == 0:
        B = N
        X, F, out = np.zeros_like(B), 2.0 * N, []
        for _ in range(K + 1):
            out.append(Cm @ X)
            X = Mx @ X + F
        return np.array(out).transpose(0, 2, 1).ravel()
    W = (U[:, :-1] + U[:, 1:]).transpose(1, 2, 0)            # (K, m, S)
    X, out = np.zeros((Mx.shape[0], U.shape[0])), []
    for k in range(K + 1):
        out.append(Cm @ X)
        if k < K:
            X = Mx @ X + N @ W[k]
    return np.array(out).transpose(2, 0, 1).ravel()


for n in args.n:
    E, A, B, Cm = system(n)
    ops = [ctx.upload(M) for M in (E, A, B, Cm)]
    t0 = time.perf_counter()
    Mx, Nx = host_setup(E, A, B)
    t_setup = 1e3 * (time.perf_counter() - t0)            # the host's M and N: once per order, added to every host time
    for K in args.K:
        rng = np.random.default_rng(K)
        for kind, S in [(0, 0)] + [(2, s) for s in args.S]:
            U = rng.standard_normal((max(S, 1), K + 1, M_))
            what = "step" if kind == 0 else f"simulate S={S}"
            if args.only_default:
                call(ops, K, kind, U, 0)
                t, (_, info) = timed(lambda: call(ops, K, kind, U, 0))
                print(f"n={n} K={K} {what}: default {t:.1f} ms, info {info}", flush=True)
                continue
            Kc, Kh = min(K, args.chain_max), min(K, args.host_max)
            variants = [("default", 0, K)] + [(f"block={b}", b, K) for b in args.blocks] + [("block=1", 1, Kc)]
            times = {nm: [] for nm, _, _ in variants}
            Us = {Kv: np.ascontiguousarray(U[:, :Kv + 1]) for Kv in {K, Kc, Kh}}
            th, infos, Ys = [], {}, {}
            for rnd in range(args.rounds + 1):                        # round 0 warms up
                for nm, b, Kv in variants:
                    t, (Y, info) = timed(lambda: call(ops, Kv, kind, Us[Kv], b))
                    infos[nm], Ys[nm] = info, Y
                    if rnd:
                        times[nm].append(t * K / Kv)
                t0 = time.perf_counter()
                Yh = host(Mx, Nx, Cm, Kh, kind, Us[Kh])
                if rnd:
                    th.append(t_setup + 1e3 * (time.perf_counter() - t0) * K / Kh)
            Yc = call(ops, Kh, kind, Us[Kh], 0)[0]
            dist = np.abs(Yc - Yh).max() / np.abs(Yh).max()
            best = min(times["default"])
            print(f"n={n} K={K} {what}: " + "; ".join(f"{nm} {fmt(v)} ms (best {min(v):.1f}, L={infos[nm][0]}, launches {infos[nm][3]}"
                                                         f"{', scaled from ' + str(Kv) if Kv != K else ''})" for (nm, _, Kv), v in zip(variants, times.values())) +
                  f"; host {fmt(th)} ms (best {min(th):.1f}, of which M and N {t_setup:.1f}{', loop scaled from ' + str(Kh) if Kh != K else ''}); block=1 / default {min(times['block=1']) / best:.2f} x, "
                  f"host / default {min(th) / best:.2f} x; max distance default to host over {Kh} steps {dist:.1e}", flush=True)
            ctx.prof_enable(True); ctx.prof_reset()
            call(ops, K, kind, U, 0)
            prof = ctx.prof_stats()
            ctx.prof_enable(False)
            tot = sum(v["ms"] for v in prof.values())
            print("   kernel timers: " + ", ".join(f"{k} {v['ms']:.2f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])) +
                  f"; total {tot:.2f} ms", flush=True)
