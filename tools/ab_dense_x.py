"""A/B of the low-rank Ros1/Ros2 time loops (gdre_solve: the dense-X step, the block-list loop, the residual-recurrence loop) between two
builds of the library.  One process runs the case list below under whichever library DRE_HIP_LIB names (default: the in-tree build) and
writes, per case, the raw arrays (every K(t_i), the factors of the final X, per Lyapunov solve the residual-norm history and the shifts) to
OUT.npz and everything else to OUT.json: per Lyapunov solve iters / converged / warnings / rhs_cols, error codes and messages, and the
profiler's per-tag (launches, bytes, flops).
  DRE_HIP_LIB=/path/to/parent/libdre_hip.so python tools/ab_dense_x.py --out /tmp/ab/parent_1
  DRE_HIP_LIB=/path/to/parent/libdre_hip.so python tools/ab_dense_x.py --out /tmp/ab/parent_2
  python tools/ab_dense_x.py --out /tmp/ab/new
  python tools/ab_dense_x.py --compare /tmp/ab/parent_1 /tmp/ab/parent_2 /tmp/ab/new
Use one fresh process per library.  `--compare P1 P2 NEW` exits 1 on any difference that is not allowed:
  * a case on which the parent's two runs agree byte for byte (arrays, counts, messages, per-tag launches) must agree byte for byte
    between P1 and NEW;
  * a case on which the parent differs from itself (the warm-started compression takes over at a step decided by hipEventQuery on a helper
    stream) is compared by D.delta of every K(t_i) against P1, bound 10 x the largest P1-against-P2 delta of that case (two runs are one
    sample of that spread), and by the iteration counts of every Lyapunov solve, which must lie within the parent's own range +- 1.
`--compare A B` is the plain byte check of two records."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def delta(a, b):            # D.delta, without loading the library
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    return 0.0 if max(na, nb) == 0.0 else float(np.linalg.norm(a - b) / max(na, nb))


def case_arrays(z, name):
    return {f: z[f] for f in z.files if f.startswith(name + "/")}


def same_bytes(x, y):
    return sorted(x) == sorted(y) and all(x[f].shape == y[f].shape and x[f].tobytes() == y[f].tobytes() for f in x)


def k_deltas(x, y, name):
    ks = sorted(f for f in x if f.startswith(name + "/K"))
    if ks != sorted(f for f in y if f.startswith(name + "/K")) or any(x[f].shape != y[f].shape for f in ks):
        return None
    return [delta(x[f], y[f]) for f in ks]


def compare(p1, p2, new):
    j1, j2, jn = (json.load(open(p + ".json")) for p in (p1, p2 or p1, new))
    z1, z2, zn = (np.load(p + ".npz") for p in (p1, p2 or p1, new))
    bad, loose = [], []
    if not (list(j1) == list(j2) == list(jn)):
        bad.append("case lists differ")
    for name in j1:
        if name not in j2 or name not in jn:
            continue
        a1, a2, an = case_arrays(z1, name), case_arrays(z2, name), case_arrays(zn, name)
        if j1[name] == j2[name] and same_bytes(a1, a2):
            if j1[name] != jn[name]:
                keys = [k for k in sorted(set(j1[name]) | set(jn[name])) if j1[name].get(k) != jn[name].get(k)]
                bad.append(f"{name}: {keys} differ" + "".join(f"\n    {k}: {j1[name].get(k)!r}\n    vs {jn[name].get(k)!r}" for k in keys))
            if not same_bytes(a1, an):
                dk = k_deltas(a1, an, name)
                bad.append(f"{name}: arrays differ (largest delta of K(t): {max(dk) if dk else 'shapes differ'})")
            continue
        # the parent does not reproduce itself on this case
        dpp, dpn = k_deltas(a1, a2, name), k_deltas(a1, an, name)
        it1, it2, itn = ([g["iters"] for g in j[name].get("gales", [])] for j in (j1, j2, jn))
        line = f"{name}: parent differs from itself"
        if dpp is None or dpn is None or not (len(it1) == len(it2) == len(itn)) or j1[name]["error"] != jn[name]["error"] or j2[name]["error"] != jn[name]["error"]:
            bad.append(line + ": shapes, solve counts or errors differ")
            continue
        spread = max(dpp)
        out_of_range = [(i, a, b, c) for i, (a, b, c) in enumerate(zip(it1, it2, itn)) if not min(a, b) - 1 <= c <= max(a, b) + 1]
        line += (f"; K(t): parent spread {spread:.3e}, new against parent {max(dpn):.3e} (bound {10 * spread:.3e}); iterations: parent {sum(it1)} / {sum(it2)}, "
                 f"new {sum(itn)}, {len(out_of_range)} solves outside the parent's range +- 1")
        loose.append(line)
        if not max(dpn) <= 10 * spread or out_of_range:
            bad.append(line + "".join(f"\n    solve {i}: parent {a}, {b}, new {c}" for i, a, b, c in out_of_range[:10]))
    print(f"{p1}" + (f", {p2}" if p2 else "") + f" vs {new}: {len(j1)} cases, {len(j1) - len(loose)} byte checks, {len(loose)} within the parent's spread, {len(bad)} failures")
    for line in loose:
        print("  (spread) " + line)
    for line in bad:
        print("  FAILED " + line)
    return 1 if bad else 0


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--compare", nargs="+", metavar="RECORD", help="A B: byte check; P1 P2 NEW: parent twice, then the new build")
ap.add_argument("--skip-5177", action="store_true", help="leave out the residual-recurrence case (SteelProfile(5177))")
args = ap.parse_args()
if args.compare:
    if len(args.compare) not in (2, 3):
        ap.error("--compare takes two or three records")
    sys.exit(compare(args.compare[0], args.compare[1] if len(args.compare) == 3 else None, args.compare[-1]))
if not args.out:
    ap.error("--out or --compare")

import dre_amd as D

ctx = D.default_context()
meta, arrays = {}, {}
_problems = {}


def problem(n, nsteps, dt=-100.0):
    if n not in _problems:
        d = D.steel_profile(n)
        L, Dm = D.initial_value(d)
        _problems[n] = (d, D.lowrank(L, Dm), list(np.load(os.path.join(ROOT, "tests", "golden", f"heuristic_shifts_{n}.npy"))))
    d, X0, shifts = _problems[n]
    return D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4500.0 + dt * nsteps)), shifts


def case(name, nsteps, n=371, order=1, dt=-100.0, options=None, **adi):
    """one solve under the kernel timers; what it returns, what it raises and the launches it made go on record"""
    assert name not in meta, name
    prob, shifts = problem(n, nsteps, dt)
    alg = (D.Ros1 if order == 1 else D.Ros2)(D.ADI(shifts=D.Shifts.Cyclic(shifts), warn_convergence=False, **adi))
    m = dict(error=[], options=options or {})
    with ctx.options(**(options or {})):
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            sol, st = D.solve_gdre(prob, alg, dt=dt, ctx=ctx, return_stats=True)
            arrays[name + "/t"] = np.asarray(sol.t)
            for i, K in enumerate(sol.K):
                arrays[f"{name}/K{i}"] = np.ascontiguousarray(K)
            X = sol.X[-1]
            for b, (al, Lb, Db) in enumerate(zip(X.alphas, X.Ls, X.Ds)):
                arrays[f"{name}/X/alpha{b}"] = np.asarray(al, dtype=float)
                arrays[f"{name}/X/L{b}"] = np.ascontiguousarray(Lb)
                arrays[f"{name}/X/D{b}"] = np.ascontiguousarray(Db)
            m["adi_iters"], m["factorizations"] = int(st["adi_iters"]), int(st["factorizations"])
            m["gales"] = []
            for j, g in enumerate(st["gales"]):
                m["gales"].append(dict(iters=g["iters"], converged=g["converged"], warnings=g["warnings"], rhs_cols=g["rhs_cols"]))
                arrays[f"{name}/gale{j}/norms"] = np.asarray(g["norms"], dtype=float)
                arrays[f"{name}/gale{j}/norm_iters"] = np.asarray(g["norm_iters"])
                arrays[f"{name}/gale{j}/shifts"] = np.asarray(g["shifts"])
                arrays[f"{name}/gale{j}/res_abstol"] = np.array([g["res_norm"], g["abstol"]])
        except D.DREError as e:
            m["error"].append([e.code, str(e)])
        ctx.sync()
        m["prof"] = {k: [v["launches"], v["bytes"], v["flops"]] for k, v in sorted(ctx.prof_stats().items())}
        ctx.prof_enable(False)
    meta[name] = m
    its = [g["iters"] for g in m.get("gales", [])]
    print(f"{name}: {'error ' + repr(m['error']) if m['error'] else 'ok'}; iterations {its}; {sum(v[0] for v in m['prof'].values())} launches; "
          + ", ".join(f"{t} {m['prof'][t][0]}" for t in ("warm_project", "adi_group_iter", "adi_fast_iter") if t in m["prof"]), flush=True)


# ---- default options: the dense-X step from the first dense step of a run (single-iteration chain, group base on the parked thread) to the
# ---- steady warm-started steps of the benchmark's configuration
for k in (1, 2, 3, 6):
    case(f"default/{k}_steps", k)
case("default/45_steps", 45, maxiters=100)
# ---- option legs
for opt in (dict(x_side_stream=0), dict(side_prefetch=1), dict(dense_warm=0), dict(dense_warm=2), dict(dense_warm=3), dict(adi_group=0),
            dict(dense_x_max_k=16),                               # the first dense step refuses (64 columns): back to the generic ADI with the side stream on
            dict(dense_x_max_k=100),                              # the second one does (144 columns): mid-run, X goes back to the factored form
            dict(final_x_lazy=0), dict(final_x_lazy=1),
            dict(x_compress_every=3, dense_x_max_n=0)):          # the block-list loop with its side job
    case("option/" + ",".join(f"{k}={v}" for k, v in opt.items()), 6, options=opt)
# (the warm path needs three dense steps and a finished eigenbasis: 6 steps may end before it; 20 steps with the warm variants reach it)
for w in (2, 3):
    case(f"option/dense_warm={w}/20_steps", 20, options=dict(dense_warm=w))
case("option/side_prefetch=1/20_steps", 20, options=dict(side_prefetch=1))
# ---- ADI options
case("adi/compression_interval=2", 6, compression_interval=2)                     # several chunks per solve
case("adi/maxiters=3", 6, maxiters=3)                                             # unconverged: warning bit
case("adi/maxiters=60,compression_interval=50", 6, maxiters=60, compression_interval=50)      # a chunk above 48 iterations: the late X update
# ---- a failing leg: every factorisation of the cycle is refused (pivot growth beyond the limit) by the side set-up of the first dense step,
# ---- after the main stream's assembly was enqueued (on one stream: the side context keeps its own limit); then an ordinary solve
case("failing/in_side_setup", 3, options=dict(pivot_growth_fail=1e-300, x_side_stream=0))
case("failing/in_side_setup/then_ordinary", 3)
# ---- Ros2 (generic path, two Lyapunov solves per step)
case("ros2/3_steps", 3, order=2)
# ---- the residual-recurrence loop (two parked threads)
if not args.skip_5177:
    case("recurrence/5177/3_steps", 3, n=5177)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.savez(args.out + ".npz", **arrays)
json.dump(meta, open(args.out + ".json", "w"), indent=1)
print(f"{len(meta)} cases, {len(arrays)} arrays -> {args.out}.npz, {args.out}.json (library: {os.environ.get('DRE_HIP_LIB', 'in-tree')})")
