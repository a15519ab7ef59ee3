"""Symmetric eigensolver timing: Householder + QL (`dre_sym_eig`, always method 0) against the whole-device block Jacobi solver
(`dre_sym_eig_jacobi`) on the matrices `FactoredSign`'s compressions really diagonalise, operands resident on the device.

Inputs: one `solve_lr` on SteelProfile(n) for every `--dump-n` (default 371 and 1357: the first Ros1 step's operator and right-hand side, as
in tools/time_factored_sign.py) runs with DRE_SYM_EIG_DUMP set, which makes the library write every matrix that reaches its eigensolver to
a file; of each run the matrices of the smallest, the median and the largest order are timed.  Plus a random symmetric matrix of order 704
(full rank: no early termination in the tridiagonalisation).  The two methods are alternated over `--rounds` rounds after a warm-up round,
in ONE process, and method 0 is timed twice per round: the spread of method 0 against itself is the yardstick for any difference.  Then,
under the library's kernel timers, the split per tag of one call of each.  For the launches per call run this under `rocprofv3
--kernel-trace --stats -d <dir> -o eig -- python tools/time_sym_eig.py --rounds 1 --dump-n 371`.
  python tools/time_sym_eig.py [--rounds 3] [--dump-n n ...] [--no-random]"""
import argparse, ctypes as C, glob, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import dre_amd as D
from dre_amd import device as dev

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dump-n", type=int, nargs="*", default=[371, 1357])
ap.add_argument("--no-random", action="store_true")
args = ap.parse_args()
ctx = D.default_context()


def dumped(n):
    """the matrices one solve_lr at SteelProfile(n) hands to the eigensolver: [(order, S), ...] in call order"""
    d = D.steel_profile(n)
    L0, D0 = D.initial_value(d)
    E, A, B, Cm = d.E.toarray(), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    tau, q = 100.0, Cm.shape[0]
    BtLD, EtL = (B.T @ L0) @ D0, E.T @ L0
    F = A - E / (2.0 * tau) - B @ (BtLD @ EtL.T)
    G = np.hstack([Cm.T, EtL])
    S = np.zeros((G.shape[1],) * 2)
    S[:q, :q] = np.eye(q)
    S[q:, q:] = BtLD.T @ BtLD + D0 / tau
    Ed, Fd, Gd, Sd = (ctx.upload(M) for M in (E, F, G, S))
    sign = D.SignFactorization(Ed, Fd, ctx=ctx)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["DRE_SYM_EIG_DUMP"] = tmp
        try:
            sign.solve_lr(Gd, Sd, None, 256, 1, download=False)
            ctx.sync()
        finally:
            del os.environ["DRE_SYM_EIG_DUMP"]
        files = sorted(glob.glob(os.path.join(tmp, "S_*.f64")), key=lambda f: int(os.path.basename(f).split("_")[1]))
        for f in files:
            o = int(os.path.basename(f).split("_")[2].split(".")[0])
            out.append((o, np.fromfile(f).reshape(o, o, order="F")))
    sign.close()
    return out


def random_sym(q, seed):
    M = np.random.default_rng(seed).standard_normal((q, q))
    return 0.5 * (M + M.T)


def call(method, Ad):
    wp, vp = C.c_void_p(), C.c_void_p()
    ii = (C.c_int64 * 2)()
    ctx.sync()
    t = time.perf_counter()
    if method == 1:
        ctx.chk(ctx.lib.dre_sym_eig_jacobi(ctx.ptr, Ad.ptr, 0.0, C.byref(wp), C.byref(vp), ii))
    else:
        ctx.chk(ctx.lib.dre_sym_eig(ctx.ptr, Ad.ptr, 4.0, C.byref(wp), C.byref(vp)))
    ctx.sync()
    ms = 1e3 * (time.perf_counter() - t)
    w, V = dev.DenseMatrix(ctx, wp), dev.DenseMatrix(ctx, vp)
    return ms, w, V, (int(ii[0]), int(ii[1]))


inputs = []
for n in args.dump_n:
    mats = dumped(n)
    orders = [o for o, _ in mats]
    print(f"solve_lr at n={n}: {len(mats)} eigenproblems, orders {min(orders)} .. {max(orders)}", flush=True)
    by_order = sorted(range(len(mats)), key=lambda i: orders[i])
    for i in sorted({by_order[0], by_order[len(by_order) // 2], by_order[-1]}):
        inputs.append((f"n={n} compression {i} (order {orders[i]})", 0.5 * (mats[i][1] + mats[i][1].T)))
if not args.no_random:
    inputs.append(("random 704", random_sym(704, 704)))
for name, S in inputs:
    Ad = ctx.upload(S)
    t = {0: [], "0 again": [], 1: []}
    for rnd in range(args.rounds + 1):                    # round 0 warms up
        a, w0, _, _ = call(0, Ad)
        b, w1, V1, st = call(1, Ad)
        a2, _, _, _ = call(0, Ad)
        if rnd:
            t[0].append(a); t[1].append(b); t["0 again"].append(a2)
    kept = w0.numpy().size
    w1, V1 = w1.numpy().ravel(), V1.numpy()
    res = np.linalg.norm(S @ V1 - V1 * w1) / np.linalg.norm(S)
    fmt = lambda v: "/".join(f"{x:.2f}" for x in v)
    print(f"{name}: QL {fmt(t[0])} ms (best {min(t[0]):.2f}, {kept} eigenpairs kept), QL again {fmt(t['0 again'])} ms (best {min(t['0 again']):.2f}), "
          f"Jacobi {fmt(t[1])} ms (best {min(t[1]):.2f}; {st[0]} sweeps, {st[1]} rounds, residual {res:.1e})", flush=True)
    for method in (0, 1):
        ctx.prof_enable(True); ctx.prof_reset()
        call(method, Ad)
        prof = ctx.prof_stats()
        ctx.prof_enable(False)
        print(f"    method {method}: " + ", ".join(f"{k} {v['ms']:.2f} ms / {v['launches']}" for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"])[:6]))
