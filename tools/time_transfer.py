"""Timing of the two methods of the frequency response: `dre_freq_response` (method="embedding": the real form of order 2n) against
`dre_transfer_eval` at s = i w (method="complex": the complex Gauss-Jordan panel) on the systems and shapes of tools/time_freq_response.py
(K = 60, m = 7, q = 6).  ONE process, operands resident on the device, a warm-up round, then `--rounds` alternated rounds, the best of the
rounds; orders above 2048 run the complex method alone (`--n-complex`, K = `--K-complex`).  Then, under the library's kernel timers, the panel /
update / product shares of each method's call.
  python tools/time_transfer.py [--rounds 3] [--K 60] [--n 371 1024 2048] [--n-complex 4096] [--K-complex 4] [--chunk 0]"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--K", type=int, default=60)
ap.add_argument("--n", type=int, nargs="*", default=[371, 1024, 2048])
ap.add_argument("--n-complex", type=int, nargs="*", default=[4096])
ap.add_argument("--K-complex", type=int, default=4)
ap.add_argument("--chunk", type=int, default=0)
args = ap.parse_args()
ctx = D.default_context()
lib = ctx.lib
pd, pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
fmt = lambda v: "/".join(f"{x:.1f}" for x in v)


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


def call(method, ops, omega, q, m):
    K = len(omega)
    re, im, st, info = np.zeros(K * q * m), np.zeros(K * q * m), np.zeros(K, dtype=np.int32), (C.c_int64 * 2)()
    tail = (args.chunk, re.ctypes.data_as(pd), im.ctypes.data_as(pd), st.ctypes.data_as(pi32), info)
    if method == "complex":
        zero = np.zeros(K)
        ctx.chk(lib.dre_transfer_eval(ctx.ptr, *(o.ptr for o in ops), K, zero.ctypes.data_as(pd), omega.ctypes.data_as(pd), *tail))
    else:
        ctx.chk(lib.dre_freq_response(ctx.ptr, *(o.ptr for o in ops), K, omega.ctypes.data_as(pd), *tail))
    assert not st.any()
    return (re + 1j * im).reshape(K, m, q).transpose(0, 2, 1), int(info[0]), int(info[1])


def shares(method, ops, omega, q, m):
    """the kernel timers of one call: panel (and interchanges), update, everything else"""
    ctx.prof_enable(True); ctx.prof_reset()
    call(method, ops, omega, q, m)
    prof = ctx.prof_stats()
    ctx.prof_enable(False)
    tot = sum(v["ms"] for v in prof.values())
    pre = "batch_cgj" if method == "complex" else "batch_gj"
    panel = sum(v["ms"] for k, v in prof.items() if k in (pre + "_panel", pre + "_unpivot"))
    update = sum(v["ms"] for k, v in prof.items() if k == pre + "_update")
    pct = lambda x: 100.0 * x / max(tot, 1e-9)
    return (f"{method}: panel {pct(panel):.1f} %, update {pct(update):.1f} %, products and the rest {pct(tot - panel - update):.1f} % of {tot:.1f} ms ("
            + ", ".join(f"{k} {v['ms']:.1f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])) + ")")


dist = lambda X, Y: max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(X, Y))
for n in args.n + args.n_complex:
    both = n in args.n
    K = args.K if both else args.K_complex
    omega = np.logspace(-5.0, 3.0, K)
    E, A, B, Cm = system(n)
    m, q = B.shape[1], Cm.shape[0]
    ops = [ctx.upload(M) for M in (E, A, B, Cm)]
    te, tc = [], []
    for rnd in range(args.rounds + 1):                        # round 0 warms up
        if both:
            a, (He, _, _) = timed(lambda: call("embedding", ops, omega, q, m))
        b, (Hc, chunk, chunks) = timed(lambda: call("complex", ops, omega, q, m))
        if rnd:
            tc.append(b)
            if both:
                te.append(a)
    line = f"n={n} K={K} (m={m}, q={q}): complex {fmt(tc)} ms (best {min(tc):.1f}, {min(tc) / K:.2f} ms per frequency, chunk {chunk} x {chunks})"
    if both:
        line += (f"; embedding {fmt(te)} ms (best {min(te):.1f}, {min(te) / K:.2f} ms per frequency); embedding / complex = {min(te) / min(tc):.2f} x; "
                 f"max distance between the two {dist(Hc, He):.1e}")
    print(line, flush=True)
    for method in (("embedding", "complex") if both else ("complex",)):
        print("   " + shares(method, ops, omega, q, m), flush=True)
