"""A/B of the low-rank ADI (csrc/engine.hip: adi_begin / adi_advance / adi_finish) between two builds of the library, in the form of
tools/ab_dense_x.py.  One process runs the case list below under whichever library DRE_HIP_LIB names (default: the in-tree build) and
writes, per case, the raw arrays (the factors of X and X itself, every K(t_i) of a time loop, per Lyapunov solve the residual-norm history
with norm_iters and the shifts) to OUT.npz and everything else to OUT.json: per Lyapunov solve iters / converged / warnings / rhs_cols,
error codes and messages, and the profiler's per-tag (launches, bytes, flops).
  DRE_HIP_LIB=/path/to/parent/libdre_hip.so python tools/ab_adi.py --out /tmp/ab/parent_1
  DRE_HIP_LIB=/path/to/parent/libdre_hip.so python tools/ab_adi.py --out /tmp/ab/parent_2
  python tools/ab_adi.py --out /tmp/ab/new
  python tools/ab_adi.py --compare /tmp/ab/parent_1 /tmp/ab/parent_2 /tmp/ab/new
Use one fresh process per library.  `--compare P1 P2 NEW` exits 1 on any difference that is not allowed:
  * a case on which the parent's two runs agree byte for byte (arrays, counts, messages, per-tag launches) must agree byte for byte
    between P1 and NEW;
  * a case on which the parent differs from itself is compared by D.delta of every K(t_i) (a single Lyapunov solve: of X) against P1, bound
    10 x the largest P1-against-P2 delta of that case (two runs are one sample of that spread), and by the iteration counts of every
    Lyapunov solve, which must lie within the parent's own range +- 1.
`--compare A B` is the plain byte check of two records.
The cases are the paths through the ADI: single-use factors with the batched and the one-by-one look-ahead and complex pairs (Projection
shifts), the dense-inverse step, the batched SMW set-up and the fast chain (Ros1 with dense_x_max_n = 0), fan groups on one rank and sharded
by shift over emulated ranks, the column-sharded step, Cyclic lists with conjugate pairs, Heuristic shifts, a user-defined strategy, user
inner solvers, the stepwise protocol, a failing leg and Ros2.  The fan cases print their fan_spmm_mix launches: 0 there means the size is
too small for the fan path and the case list needs a larger pencil."""
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
                bad.append(f"{name}: arrays differ (largest delta of K(t) / X: {max(dk) if dk else 'shapes differ'})")
            continue
        # the parent does not reproduce itself on this case
        dpp, dpn = k_deltas(a1, a2, name), k_deltas(a1, an, name)
        it1, it2, itn = ([g["iters"] for g in j[name].get("gales", [])] for j in (j1, j2, jn))
        line = f"{name}: parent differs from itself"
        if not dpp or not dpn or not (len(it1) == len(it2) == len(itn)) or j1[name]["error"] != jn[name]["error"] or j2[name]["error"] != jn[name]["error"]:
            bad.append(line + ": shapes, solve counts or errors differ")
            continue
        spread = max(dpp)
        out_of_range = [(i, a, b, c) for i, (a, b, c) in enumerate(zip(it1, it2, itn)) if not min(a, b) - 1 <= c <= max(a, b) + 1]
        line += (f"; K(t) / X: parent spread {spread:.3e}, new against parent {max(dpn):.3e} (bound {10 * spread:.3e}); iterations: parent {sum(it1)} / {sum(it2)}, "
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
ap.add_argument("--n", type=int, default=371, help="SteelProfile size of the cases (a golden shift list must exist for it)")
args = ap.parse_args()
if args.compare:
    if len(args.compare) not in (2, 3):
        ap.error("--compare takes two or three records")
    sys.exit(compare(args.compare[0], args.compare[1] if len(args.compare) == 3 else None, args.compare[-1]))
if not args.out:
    ap.error("--out or --compare")

import scipy.sparse.linalg as spla
import dre_amd as D

ctx = D.default_context()
meta, arrays = {}, {}
N = args.n
d = D.steel_profile(N)
L0, Dm0 = D.initial_value(d)
X0 = D.lowrank(L0, Dm0)
SHIFTS = [float(v) for v in np.load(os.path.join(ROOT, "tests", "golden", f"heuristic_shifts_{N}.npy"))]
# a Cyclic list with conjugate pairs between the real shifts: the pairs sit beside the golden values they replace
PAIRS = []
for i, s in enumerate(SHIFTS):
    PAIRS += [complex(s, 0.3 * s), complex(s, -0.3 * s)] if i % 3 == 1 else [s]


def put_x(name, X):
    arrays[name + "/K0"] = np.ascontiguousarray(X.dense())           # (the spread rule of --compare looks at the arrays called K*)
    for b, (al, Lb, Db) in enumerate(zip(X.alphas, X.Ls, X.Ds)):
        arrays[f"{name}/X/alpha{b}"] = np.asarray(al, dtype=float)
        arrays[f"{name}/X/L{b}"] = np.ascontiguousarray(Lb)
        arrays[f"{name}/X/D{b}"] = np.ascontiguousarray(Db)


def put_gale(name, j, g):
    arrays[f"{name}/gale{j}/norms"] = np.asarray(g["norms"], dtype=float)
    arrays[f"{name}/gale{j}/norm_iters"] = np.asarray(g["norm_iters"])
    arrays[f"{name}/gale{j}/shifts"] = np.asarray(g["shifts"])
    arrays[f"{name}/gale{j}/res_abstol"] = np.array([g["res_norm"], g["abstol"]])
    return dict(iters=int(g["iters"]), converged=bool(g["converged"]), warnings=int(g["warnings"]), rhs_cols=int(g["rhs_cols"]))


def record(name, options, body):
    """one case under the kernel timers; what it returns, what it raises and the launches it made go on record"""
    assert name not in meta, name
    m = dict(error=[], options=options or {})
    with ctx.options(**(options or {})):
        ctx.prof_enable(True); ctx.prof_reset()
        try:
            body(m)
        except D.DREError as e:
            m["error"].append([e.code, str(e)])
        ctx.sync()
        m["prof"] = {k: [v["launches"], v["bytes"], v["flops"]] for k, v in sorted(ctx.prof_stats().items())}
        ctx.prof_enable(False)
    meta[name] = m
    its = [g["iters"] for g in m.get("gales", [])]
    print(f"{name}: {'error ' + repr(m['error']) if m['error'] else 'ok'}; iterations {its}; {sum(v[0] for v in m['prof'].values())} launches; "
          + ", ".join(f"{t} {m['prof'][t][0]}" for t in ("fan_spmm_mix", "adi_fast_iter", "comm_allgather_w", "comm_allgather_v") if t in m["prof"]), flush=True)
    return m


def gale_problem(lowrank_update):
    A = d.A
    if lowrank_update:                          # the Rosenbrock situation: F = A - B (1e-4 B'), rank 7
        A = D.lr_update(d.A, -1.0, d.B, 1e-4 * np.asarray(d.B).T)
    return D.GALEProblem(d.E, A, D.lowrank(np.asarray(d.C).T, np.eye(np.asarray(d.C).shape[0])))


def gale_case(name, lowrank_update=True, options=None, **adi):
    def body(m):
        X, info = D.solve_gale(gale_problem(lowrank_update), D.ADI(warn_convergence=False, **adi), return_info=True)
        put_x(name, X)
        m["gales"] = [put_gale(name, 0, info)]
    return record(name, options, body)


def loop_case(name, nsteps, order=1, dt=-100.0, options=None, **adi):
    def body(m):
        prob = D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4500.0 + dt * nsteps))
        alg = (D.Ros1 if order == 1 else D.Ros2)(D.ADI(shifts=D.Shifts.Cyclic(SHIFTS), warn_convergence=False, **adi))
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
        m["gales"] = [put_gale(name, j, g) for j, g in enumerate(st["gales"])]
    return record(name, options, body)


class SpLU(D.BlockLinearSolver):
    def solve(self, prob):
        return spla.splu(prob.A.tocsc()).solve(prob.B.astype(prob.A.dtype))


class Dummy(D.Shifts.Strategy):
    """every batch is the same list (the reference's test strategy)"""

    def __init__(self, values):
        self.values = list(values)

    def take_many(self, hist):
        return self.values


import warnings
warnings.simplefilter("ignore")           # ("ADI did not converge", "Increment is zero": on record through the warning bits)

# ---- one Lyapunov solve with default (Projection) shifts: single-use factors, the batched and the one-by-one look-ahead, complex pairs
for lr in (False, True):
    for opt in ({}, dict(prefetch_batch=0), dict(setup_streams=0)):
        gale_case(f"projection/{'lowrank' if lr else 'plain'}/" + (",".join(f"{k}={v}" for k, v in opt.items()) or "default"), lowrank_update=lr, options=opt)
# ---- shift and solver variants
gale_case("cyclic/pairs", shifts=D.Shifts.Cyclic(PAIRS), maxiters=60)
gale_case("cyclic/pairs/multifrontal", shifts=D.Shifts.Cyclic(PAIRS), maxiters=60, options=dict(dense_inverse_max_n=0))
gale_case("heuristic", shifts=D.Shifts.Cyclic(D.Shifts.Heuristic(10, 10, 10)))
gale_case("user_strategy", shifts=Dummy(SHIFTS))
gale_case("user_strategy/pairs", shifts=Dummy(PAIRS), maxiters=60)
gale_case("inner/Backslash", shifts=D.Shifts.Cyclic(PAIRS), maxiters=30, inner_alg=D.Backslash())
gale_case("inner/SMW(user,Backslash)", shifts=D.Shifts.Cyclic(PAIRS), maxiters=30, inner_alg=D.ShermanMorrisonWoodbury(SpLU(), D.Backslash()))
gale_case("inner/user", shifts=D.Shifts.Cyclic(PAIRS), maxiters=30, inner_alg=SpLU())


# ---- ADISolver stepped one shift at a time against solve
def stepped(name, options=None, **adi):
    def body(m):
        prob, alg = gale_problem(True), D.ADI(warn_convergence=False, **adi)
        s = D.init(prob, alg, ctx=ctx)
        its = []
        while not D.isdone(s):
            D.step_(s)
            its.append(int(s.state()["iters"]))
        arrays[name + "/stepped_iters"] = np.asarray(its)
        put_x(name, s.X)
        m["gales"] = [put_gale(name, 0, s.info)]
        s2 = D.init(prob, alg, ctx=ctx)
        put_x(name + "/solve", D.solve_(s2))
        m["gales"].append(put_gale(name, 1, s2.info))
    return record(name, options, body)


stepped("stepped/projection")
stepped("stepped/cyclic_pairs", shifts=D.Shifts.Cyclic(PAIRS), maxiters=60)
stepped("stepped/cyclic/multifrontal", shifts=D.Shifts.Cyclic(SHIFTS), options=dict(dense_inverse_max_n=0))

# ---- Ros1, 3 steps, the generic ADI on the dense-inverse path: the dense step in the first solve, the batched SMW set-up and the fast chain
# ---- from the second step
loop_case("ros1/dense_inverse", 3, options=dict(dense_x_max_n=0))
loop_case("ros1/dense_inverse/adi_group=0", 3, options=dict(dense_x_max_n=0, adi_group=0))
# ---- Ros1, 3 steps on the multifrontal path: fan groups
MF = dict(dense_inverse_max_n=0, dense_x_max_n=0)
fan_cases = []
for fan in (8, 2, 0):
    fan_cases.append((loop_case(f"ros1/fan/adi_fan={fan}", 3, options=dict(MF, adi_fan=fan)), fan >= 2))
fan_cases.append((loop_case("ros1/fan/adi_fan_max_coef=2", 3, options=dict(MF, adi_fan_max_coef=2)), False))
fan_cases.append((loop_case("ros1/fan/compression_interval=2", 3, options=MF, compression_interval=2), True))
fan_cases.append((loop_case("ros1/fan/maxiters=3", 3, options=MF, maxiters=3), True))
# ---- the same sharded over emulated ranks: groups sharded by shift, and the column-sharded step (ctx.options puts shard_emulate back to 0)
for P in (2, 4):
    fan_cases.append((loop_case(f"ros1/fan/shard_emulate={P}", 3, options=dict(MF, shard_emulate=P)), True))
    loop_case(f"ros1/columns/shard_emulate={P}", 3, options=dict(MF, shard_emulate=P, adi_fan=0, shard_min_cols=1))
assert ctx.get_option("shard_emulate") == 0
# ---- a failing leg: every factorisation is refused (pivot growth beyond the limit); then an ordinary solve on the same context
gale_case("failing/pivot_growth", shifts=D.Shifts.Cyclic(SHIFTS), options=dict(pivot_growth_fail=1e-300))
gale_case("failing/pivot_growth/then_ordinary", shifts=D.Shifts.Cyclic(SHIFTS))
loop_case("failing/loop/pivot_growth", 2, options=dict(MF, pivot_growth_fail=1e-300))
loop_case("failing/loop/then_ordinary", 2, options=MF)
# ---- Ros2, 2 steps (two Lyapunov solves per step)
loop_case("ros2/2_steps", 2, order=2)
loop_case("ros2/2_steps/multifrontal", 2, order=2, options=MF)

no_fan = [m["options"] for m, expect in fan_cases if expect and m["prof"].get("fan_spmm_mix", [0])[0] == 0 and not m["error"]]
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.savez(args.out + ".npz", **arrays)
json.dump(meta, open(args.out + ".json", "w"), indent=1)
print(f"{len(meta)} cases, {len(arrays)} arrays -> {args.out}.npz, {args.out}.json (library: {os.environ.get('DRE_HIP_LIB', 'in-tree')})")
if no_fan:
    print(f"NO FAN GROUPS at n = {N} under {no_fan}: run the fan cases with a larger pencil (--n 1357)")
    sys.exit(2)
