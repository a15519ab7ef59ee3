"""Bit-for-bit A/B of the dense Rosenbrock drivers (dense_gdre_solve, dense_gdre_solve_adaptive, dense_gdre_solve_batched) between two
builds of the library.  One process runs the case list below under whichever library DRE_HIP_LIB names (default: the in-tree build) and
writes, per case, the raw result arrays to OUT.npz and everything else to OUT.json: times, statistics dicts, error codes and messages, and
the profiler's per-tag (launches, bytes, flops).  `--compare A B` checks np.array_equal on the arrays' bytes and equality of the rest (the
text of a memory refusal up to its free-memory figure) and exits 1 on any difference.
  DRE_HIP_LIB=/path/to/parent/libdre_hip.so python tools/ab_dense_ros.py --out /tmp/ab/parent_1
  python tools/ab_dense_ros.py --out /tmp/ab/new
  python tools/ab_dense_ros.py --compare /tmp/ab/parent_1 /tmp/ab/new
Use one fresh process per library."""
import argparse, ctypes as C, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np


def compare(a, b):
    ja, jb = json.load(open(a + ".json")), json.load(open(b + ".json"))
    za, zb = np.load(a + ".npz"), np.load(b + ".npz")
    bad = []
    if list(ja) != list(jb):
        bad.append(f"case lists differ: {sorted(set(ja) ^ set(jb))}")
    if sorted(za.files) != sorted(zb.files):
        bad.append(f"array lists differ: {sorted(set(za.files) ^ set(zb.files))}")
    for name in ja:
        if name not in jb:
            continue
        ma, mb = dict(ja[name]), dict(jb[name])
        if ma.pop("memory_refusal", False) | mb.pop("memory_refusal", False):       # "... MiB of device memory needed, <free> MiB available"
            for m in (ma, mb):
                m["error"] = [[c, re.sub(r"\d+ MiB available", "* MiB available", t)] for c, t in m["error"]]
        if ma != mb:
            keys = [k for k in sorted(set(ma) | set(mb)) if ma.get(k) != mb.get(k)]
            bad.append(f"{name}: {keys} differ" + "".join(f"\n    {k}: {ma.get(k)!r}\n    vs {mb.get(k)!r}" for k in keys))
    for f in za.files:
        if f in zb.files and (za[f].shape != zb[f].shape or za[f].tobytes() != zb[f].tobytes()):
            d = np.abs(za[f] - zb[f]).max() if za[f].shape == zb[f].shape else float("nan")
            bad.append(f"array {f}: bytes differ (shapes {za[f].shape}, {zb[f].shape}, max |difference| {d:.3e})")
    print(f"{a} vs {b}: {len(ja)} cases, {len(za.files)} arrays, {len(bad)} differences")
    for line in bad:
        print("  " + line)
    return 1 if bad else 0


ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--compare", nargs=2)
args = ap.parse_args()
if args.compare:
    sys.exit(compare(*args.compare))
if not args.out:
    ap.error("--out or --compare")

import dre_amd as D
import _adaptive_ros2_model as am
import _sign_dual_cases as dc

ctx = D.default_context()
MS = D.MatrixSign()
ROS = {1: D.Ros1, 2: D.Ros2, 3: D.Ros3, 4: D.Ros4}
meta, arrays = {}, {}


def put_solution(name, sol):
    arrays[name + "/t"] = np.asarray(sol.t)
    for i, K in enumerate(sol.K):
        arrays[f"{name}/K{i}"] = np.ascontiguousarray(K)
    for i, X in enumerate(sol.X):
        arrays[f"{name}/X{i}"] = np.ascontiguousarray(X)
    return dict(nt=len(sol.t), nK=len(sol.K), nX=len(sol.X))


def put_stats(name, st):
    st = dict(st)
    if "err" in st:
        arrays[name + "/err"] = np.asarray(st.pop("err"))
    return st


def put_result(name, res):
    """a solution, a (solution, stats) pair, a DREError of solve_batch (with its partial result), or a list of those"""
    if isinstance(res, list):
        return [put_result(f"{name}/member{b}", r) for b, r in enumerate(res)]
    if isinstance(res, D.DREError):
        return dict(member_error=[res.code, str(res)], partial=put_result(name + "/partial", res.partial) if hasattr(res, "partial") else None)
    if isinstance(res, tuple):
        return dict(solution=put_solution(name, res[0]), stats=put_stats(name, res[1]))
    return dict(solution=put_solution(name, res))


def case(name, fn, memory_refusal=False):
    """run fn under the kernel timers; what it returns, what it raises and the launches it made go on record"""
    assert name not in meta, name
    ctx.prof_enable(True); ctx.prof_reset()
    m = dict(error=[], memory_refusal=memory_refusal)
    try:
        res = fn()
        m["result"] = res if isinstance(res, (int, type(None))) else put_result(name, res)
    except D.DREError as e:
        m["error"].append([e.code, str(e)])
    if isinstance(m.get("result"), int) and m["result"] != 0:            # a raw ABI call: its code and the context's message
        m["error"].append([m["result"], ctx.lib.dre_last_error(ctx.ptr).decode()])
    m["prof"] = {k: [v["launches"], v["bytes"], v["flops"]] for k, v in sorted(ctx.prof_stats().items())}
    ctx.prof_enable(False)
    meta[name] = m
    print(f"{name}: {'error ' + repr(m['error']) if m['error'] else 'ok'}; {sum(v[0] for v in m['prof'].values())} launches", flush=True)


def fixed(E, A, B, Cm, X0, tspan, dt, order, save_state):
    return lambda: D.solve(D.GDREProblem(E, A, B, Cm, X0, tspan), ROS[order](MS), dt=dt, save_state=save_state, return_stats=True)


# ---- the fixed grid: orders 1..4 -------------------------------------------------------------------------------------------------
d = D.steel_profile(371)
L, Dm = D.initial_value(d)
Es, As, X0s = d.E.toarray(), d.A.toarray(), D.lowrank(L, Dm).dense()
for order in (1, 2, 3, 4):
    for save in (False, True):
        case(f"steel371/ros{order}/save{int(save)}", fixed(Es, As, d.B, d.C, X0s, (4500.0, 4200.0), -100.0, order, save))
E6, A6, B6, C6 = am.stiff_pencil(6, seed=3)
E33, F33, G33, _ = dc.pencil(33)                         # non-symmetric E and F; F serves as A, columns of G as B and C'
B33, C33 = np.array(G33[:, :2]), np.array(G33[:, 2:5].T)
for order in (1, 2, 3, 4):
    for tag, tspan, dt in (("backwards", (1.0, 0.0), -0.25), ("forwards", (0.0, 1.0), 0.25)):
        case(f"stiff6/ros{order}/{tag}", fixed(E6, A6, B6, C6, np.zeros((6, 6)), tspan, dt, order, True))
        case(f"nonsym33/ros{order}/{tag}", fixed(np.array(E33), np.array(F33), B33, C33, np.zeros((33, 33)), tspan, dt, order, True))
case("zero_steps", fixed(E6, A6, B6, C6, np.eye(6), (1.0, 0.9), -0.25, 2, False))
case("zero_steps/save", fixed(E6, A6, B6, C6, np.eye(6), (1.0, 0.9), -0.25, 4, True))

# ---- the adaptive cases of tests/test_gpu_dense_adaptive.py ------------------------------------------------------------------------
RTOL, ATOL, TSPAN, DT0, TSTOP = 1e-3, 1e-6, (1.0, 0.0), -0.5, 0.4
for n, seed in ((33, 2), (70, 0)):
    E, A, B, Cm = am.stiff_pencil(n, seed=seed)
    prob = D.GDREProblem(E, A, B, Cm, np.zeros((n, n)), TSPAN)
    sc = D.StepControl(rtol=RTOL, atol=ATOL, tstops=(TSTOP,))
    for save in (True, False):                          # (rejected steps: 25 at n = 33, 64 at n = 70)
        case(f"adaptive{n}/save{int(save)}", lambda: D.solve(prob, D.Ros2(MS), dt=DT0, adaptive=sc, save_state=save, return_stats=True))
    tau = am.solve(E, A, B, Cm, np.zeros((n, n)), TSPAN, DT0, rtol=RTOL, atol=ATOL, tstops=(TSTOP,)).trials[0][1]
    case(f"adaptive{n}/rejected_at_dt_min", lambda: D.solve(prob, D.Ros2(MS), dt=-tau, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, dt_min=tau, dt_max=tau)))
    case(f"adaptive{n}/max_steps", lambda: D.solve(prob, D.Ros2(MS), dt=DT0, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, max_steps=1)))
E, A, B, Cm = am.stiff_pencil(33, seed=2)
case("adaptive33/several_tstops_forwards", lambda: D.solve(D.GDREProblem(E, A, B, Cm, np.zeros((33, 33)), (0.0, 0.06)), D.Ros2(MS), dt=0.02,
                                                           adaptive=D.StepControl(rtol=1e-2, atol=1e-4, tstops=(0.01, 0.013, 0.05)),
                                                           save_state=True, return_stats=True))

# ---- ensembles --------------------------------------------------------------------------------------------------------------------
members = lambda tspan: [D.GDREProblem(Es, As, s * d.B, d.C, X0s, tspan) for s in (1.0, 0.5, 2.0)]
for order in (1, 2):
    for nb in (1, 3):
        for save in (False, True):
            case(f"batch/ros{order}/B{nb}/save{int(save)}",
                 lambda: D.solve_batch(members((4500.0, 4200.0))[:nb], ROS[order](MS), dt=-100.0, save_state=save, return_stats=True))
p = members((4500.0, 4200.0))
bad = D.GDREProblem(Es, -As, d.B, d.C, X0s, (4500.0, 4200.0))
case("batch/failing_member", lambda: D.solve_batch([p[0], bad, p[2]], D.Ros1(MS), dt=-100.0, errors="return", save_state=True, return_stats=True))
case("batch/failing_member/alone", lambda: D.solve_batch([p[0], p[2]], D.Ros1(MS), dt=-100.0, save_state=True, return_stats=True))
fm, al = meta["batch/failing_member"], meta["batch/failing_member/alone"]
same = all(np.array_equal(arrays[k], arrays[k.replace("failing_member/member2", "failing_member/alone/member1").replace("failing_member/member0", "failing_member/alone/member0")])
           for k in arrays if k.startswith("batch/failing_member/member0") or k.startswith("batch/failing_member/member2"))
meta["batch/failing_member"]["others_unchanged"] = bool(same)
print(f"batch/failing_member: the other members equal their run without the failing one: {same}", flush=True)

# ---- the refusal texts, through the C ABI -------------------------------------------------------------------------------------------
ups6 = [ctx.upload(np.asfortranarray(M)) for M in (E6, A6, B6, C6, np.zeros((6, 6)))]
ups33 = [ctx.upload(np.asfortranarray(M)) for M in (np.array(E33), np.array(F33), B33, C33, np.zeros((33, 33)))]
ups371 = [ctx.upload(np.asfortranarray(M)) for M in (Es, As, d.B, d.C, X0s)]
ctx.sync()


def abi_fixed(ups, t0=1.0, tf=0.0, dt=-0.25, order=2, maxiters=50, save=0):
    r = C.c_void_p()
    rc = ctx.lib.dre_dense_gdre_solve(ctx.ptr, *[u.ptr for u in ups], t0, tf, dt, order, save, maxiters, 0.0, 2, C.byref(r))
    if r:
        ctx.lib.dre_gdre_result_free(r)
    return rc


def abi_adaptive(ups, order=2, dt0=-0.5):
    r = C.c_void_p()
    ts = np.zeros(0)
    rc = ctx.lib.dre_dense_gdre_solve_adaptive(ctx.ptr, *[u.ptr for u in ups], 1.0, 0.0, dt0, order, 1e-3, 1e-6, 0.0, np.inf, 100,
                                               ts.ctypes.data_as(C.POINTER(C.c_double)), 0, 0, 50, 0.0, 2, C.byref(r))
    if r:
        ctx.lib.dre_gdre_result_free(r)
    return rc


def abi_batched(ups, batch, order, dt=-0.5, maxiters=50):
    arrs = [(C.c_void_p * batch)(*([u.ptr] * batch)) for u in ups]
    rs = (C.c_void_p * batch)()
    st = np.zeros(batch, dtype=np.int32)
    rc = ctx.lib.dre_dense_gdre_solve_batched(ctx.ptr, batch, *arrs, 1.0, 0.0, dt, order, 0, maxiters, 0.0, 2, rs, st.ctypes.data_as(C.POINTER(C.c_int32)))
    for r in rs:
        if r:
            ctx.lib.dre_gdre_result_free(C.c_void_p(r))
    return rc


for order in (0, 5):
    case(f"refusal/order{order}", lambda: abi_fixed(ups6, order=order))
    case(f"refusal/batched/order{order}", lambda: abi_batched(ups6, 2, order))
case("refusal/batched/order3", lambda: abi_batched(ups6, 2, 3))
case("refusal/adaptive/order1", lambda: abi_adaptive(ups6, order=1))
case("refusal/adaptive/dt0_wrong_sign", lambda: abi_adaptive(ups6, dt0=0.5))
for who, call in (("single", lambda **kw: abi_fixed(ups6, **kw)), ("batched", lambda **kw: abi_batched(ups6, 2, 1, **kw))):
    case(f"refusal/{who}/dt_zero", lambda: call(dt=0.0))
    case(f"refusal/{who}/dt_nan", lambda: call(dt=float("nan")))
    case(f"refusal/{who}/dt_wrong_sign", lambda: call(dt=0.25))
    case(f"refusal/{who}/maxiters", lambda: call(maxiters=0))
mixed = [ups6[0], ups33[1], ups6[2], ups6[3], ups6[4]]                       # A of another order
case("refusal/single/shapes", lambda: abi_fixed(mixed))
case("refusal/adaptive/shapes", lambda: abi_adaptive(mixed))
case("refusal/batched/shapes", lambda: abi_batched(mixed, 2, 1))
import torch
total = torch.cuda.get_device_properties(0).total_memory
case("refusal/batched/memory", lambda: abi_batched(ups371, min(65535, int(total // (60 * 371 * 371 * 8)) + 1), 1), memory_refusal=True)
case("refusal/single/memory", lambda: abi_fixed(ups371, dt=-1.0 / (int(total // (371 * 371 * 8)) + 1), order=1, save=1), memory_refusal=True)      # one saved state per step
case("after_the_refusals", fixed(E6, A6, B6, C6, np.zeros((6, 6)), (1.0, 0.0), -0.25, 2, False))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
np.savez(args.out + ".npz", **arrays)
json.dump(meta, open(args.out + ".json", "w"), indent=1)
print(f"{len(meta)} cases, {len(arrays)} arrays -> {args.out}.npz, {args.out}.json (library: {os.environ.get('DRE_HIP_LIB', 'in-tree')})")
