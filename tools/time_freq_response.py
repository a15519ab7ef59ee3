"""Frequency-response timing: ONE `dre_freq_response` call of K frequencies against (a) a loop of K single `dre_dense_invert` calls on the
real form [[-A, -wE], [wE, -A]] (assembled on the host and resident on the device before the clock starts; the call works in place, so the
resident matrices alternate between M and M^-1 from round to round, the same work either way) plus the three `dre_gemm` products,
and (b) the NumPy loop of tests/_balance_cases.py: transfer on the host (one complex LU solve per frequency).  Alternated over `--rounds`
rounds after a warm-up round in ONE process; operands resident on the device.

Systems: steel_profile(371, convection=3e-3) with the non-symmetric E of tests/_sign_dual_cases.py, and fixed-seed random stable pencils
E = I + 0.1 N / sqrt(n), A = -(I + 0.4 N' / sqrt(n)) E with m = 7, q = 6 at the other orders.  At large n the single-call loop holds only
`--single-max` embeddings on the device (each is 32 n^2 bytes) and its time is scaled to K.
Then, under the library's kernel timers, the share of each kernel class in the batched call.  `--only-batched` runs nothing but one warm-up and
one batched call per order (for a kernel trace of its own).
  python tools/time_freq_response.py [--rounds 3] [--K 60] [--n 371 1024 2048] [--chunk 0]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--K", type=int, default=60)
ap.add_argument("--n", type=int, nargs="*", default=[371, 1024, 2048])
ap.add_argument("--chunk", type=int, default=0)
ap.add_argument("--single-max", type=int, default=12)
ap.add_argument("--only-batched", action="store_true")
args = ap.parse_args()
ctx = D.default_context()
lib = ctx.lib
pd, pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
fmt = lambda v: "/".join(f"{x:.1f}" for x in v)
OMEGA = np.logspace(-5.0, 3.0, args.K)


def system(n):
    if n == 371:
        d = D.steel_profile(n, convection=3e-3)
        rng = np.random.default_rng(109)
        N = np.triu(rng.standard_normal((n, n)), 1)
        N /= np.linalg.norm(N, 2)
        return d.E.toarray() @ (np.eye(n) + 0.1 * N), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    rng = np.random.default_rng(n)
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    A = -(np.eye(n) + 0.4 * rng.standard_normal((n, n)) / np.sqrt(n)) @ E
    return E, A, rng.standard_normal((n, 7)), rng.standard_normal((6, n))


def timed(f):
    ctx.sync()
    t = time.perf_counter()
    out = f()
    ctx.sync()
    return 1e3 * (time.perf_counter() - t), out


def batched(ops, q, m):
    K = len(OMEGA)
    re, im, st, info = np.zeros(K * q * m), np.zeros(K * q * m), np.zeros(K, dtype=np.int32), (C.c_int64 * 2)()
    ctx.chk(lib.dre_freq_response(ctx.ptr, *(o.ptr for o in ops), K, OMEGA.ctypes.data_as(pd), args.chunk, re.ctypes.data_as(pd), im.ctypes.data_as(pd),
                                  st.ctypes.data_as(pi32), info))
    assert not st.any()
    return (re + 1j * im).reshape(K, m, q).transpose(0, 2, 1), int(info[0]), int(info[1])


def single_loop(Ms, Bp, Cre, Cim):
    """per frequency: the inversion in place, Y = M^-1 [B; 0], [C 0] Y and [0 C] Y"""
    out = []
    for M in Ms:
        ctx.chk(lib.dre_dense_invert(ctx.ptr, M.ptr, None, None))
        Y = ctx.gemm(False, False, 1.0, M, Bp)
        out.append((ctx.gemm(False, False, 1.0, Cre, Y), ctx.gemm(False, False, 1.0, Cim, Y)))
    return out


for n in args.n:
    E, A, B, Cm = system(n)
    m, q = B.shape[1], Cm.shape[0]
    ops = [ctx.upload(M) for M in (E, A, B, Cm)]
    if args.only_batched:
        batched(ops, q, m)
        t, (H, chunk, chunks) = timed(lambda: batched(ops, q, m))
        print(f"n={n} K={args.K}: batched {t:.1f} ms, chunk {chunk} x {chunks}", flush=True)
        continue
    ks = min(args.single_max, args.K)
    Ms = [ctx.upload(np.block([[-A, -w * E], [w * E, -A]])) for w in OMEGA[:ks]]
    Bp, Cre, Cim = ctx.upload(np.vstack([B, np.zeros_like(B)])), ctx.upload(np.hstack([Cm, np.zeros_like(Cm)])), ctx.upload(np.hstack([np.zeros_like(Cm), Cm]))
    tb, tl, th = [], [], []
    for rnd in range(args.rounds + 1):                        # round 0 warms up
        a, (H, chunk, chunks) = timed(lambda: batched(ops, q, m))
        b, outs = timed(lambda: single_loop(Ms, Bp, Cre, Cim))
        t0 = time.perf_counter()
        Hh = np.array([Cm @ np.linalg.solve(1j * w * E - A, B.astype(complex)) for w in OMEGA])
        c = 1e3 * (time.perf_counter() - t0)
        if rnd:
            tb.append(a); tl.append(b * args.K / ks); th.append(c)
        else:
            Hs = np.array([r.numpy() + 1j * i.numpy() for r, i in outs])      # (the first pass inverts M itself)
    dist = lambda X, Y: max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(X, Y))
    print(f"n={n} K={args.K} (2n={2 * n}, m={m}, q={q}): batched {fmt(tb)} ms (best {min(tb):.1f}, {min(tb) / args.K:.2f} ms per frequency, chunk {chunk} x {chunks}); "
          f"{ks} single inversions + products scaled to K {fmt(tl)} ms (best {min(tl):.1f}) = {min(tl) / min(tb):.2f} x; NumPy loop on the host {fmt(th)} ms "
          f"(best {min(th):.1f}) = {min(th) / min(tb):.2f} x; max distance to the host loop: batched {dist(H, Hh):.1e}, single {dist(Hs, Hh[:ks]):.1e}", flush=True)
    ctx.prof_enable(True); ctx.prof_reset()
    batched(ops, q, m)
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    tot = sum(v["ms"] for v in prof.values())
    inv = sum(v["ms"] for k, v in prof.items() if k.startswith("batch_gj"))
    print("   kernel timers: " + ", ".join(f"{k} {v['ms']:.1f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])) +
          f"; inversion {100 * inv / max(tot, 1e-9):.1f} % of {tot:.1f} ms", flush=True)
    del Ms
