#!/usr/bin/env python3
"""Headline benchmark: ADI iterations/sec + GDRE wall-clock, SteelProfile Ros1 LRSIF (BASELINE.json).

One "step" = one complete low-rank Rosenbrock-1 solve of the generalized differential Riccati equation on the
SteelProfile(n) surrogate: tspan = (4500, 0), dt = -100 (45 time steps), X0 = L(0.01 I)L', ADI with
Cyclic real shifts (real parts of Heuristic(10,20,20), tests/golden/heuristic_shifts_<n>.npy), all inputs
resident in HBM before the timed region starts.

N > 1: one process per GPU (torchrun).  Default mode `replicas` (weak scaling): every rank solves an independent replica (time steps are
sequentially dependent) and the K(t) feedback trajectories are gathered inside the timed region by the LIBRARY's
communicator (RCCL over xGMI, dre_comm_allgather on the library stream).  `--mode strong`: ONE solve, the same device-resident time loop on
every rank, the independent shifted solves of every fan group farmed over the ranks inside the library, one all-gather per group (meant for --n 5177 / 20209).

A plain run sets up, warms up, times --steps solves and prints the headline record; `--dump-outputs DIR` writes what the last timed solve
returned (K(t) and the ADI iteration count of every Lyapunov solve) as DIR/<name>.npy.

With `--full`, legs after the timed region (rank 0): `roofline` (one profiled solve, HIP events per kernel class on the library's streams),
`parity` (K(t) of the timed solve against the oracle's committed full-length fixture; the run FAILS on a mismatch), and at N = 1, n = 371 one leg
per remaining BASELINE config, each with its own roofline, parity and set-up times: `general_path` (SteelProfile(5177), 12 steps — the leg of
rounds 2-3), `general_path_45` (configs[3] at its stated 45 steps), `general_path_20209` (configs[4]: save_state, 12 steps), `ros2_1357_projection`
(configs[2]: Ros2 with the default Projection(2) shifts, complex pairs); `cpu_baseline` (the NumPy/SciPy oracle, N = 1; configs[0]'s dense
Rosenbrock solver is timed there too).

Prints ONE JSON line (rank 0).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np


# kernel-class tag of the library's timers -> symbol prefix in the rocprofv3 outputs (profiles/pmc_traffic_r02_n<n>.json)
KERNEL_SYMBOL = {"qr_panel": "k_qr_panel", "qr_panel_tsqr": "k_tsqr", "gemm_band": "k_gemm", "gemm_qr": "k_gemm", "gemm_compress": "k_gemm",
                 "gemm_gram": "k_gemm", "gemm_dinv": "k_gemm", "dense_step": "k_dense_step", "band_w": "k_band_w", "mf_solve_real": "k_mf_",
                 "mf_factor_real": "k_front_factor", "spmm_csr": "k_spmm", "band_rem": "k_band_rem", "ldlt_norm": "k_gram_norm",
                 "gemm_lrband": "k_gemm", "lrband_rows": "k_rows_blockdiag", "lrband_decide": "k_lr_", "adi_fast_iter": "k_adi_fast", "adi_group_iter": "k_adi_group",
                 "adi_fast_flush": "k_adi_fast", "band_z": "k_band_z", "band_upd": "k_band_upd", "adi_eff_stack": "k_eff_stack",
                 "gemm_xupdate": "k_gemm", "fan_spmm_mix": "k_fan_spmm_mix", "smw_apply": "k_smw_apply", "gemm_mf_top": "k_gemm_z", "gemm_sketch": "k_gemm",
                 "gemm_orth": "k_gemm", "mf_factor_complex": "k_front_factor", "mf_solve_complex": "k_mf_"}


# kernels of a timed scope that spans several kernels (roofline.traffic is summed over them)
SCOPE_SYMBOLS = {"mf_solve_real": ["k_mf_forward", "k_mf_backward", "k_top_gather", "k_gemm_z", "k_gemm_reduce_z", "k_mf_sub"]}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n", type=int, default=371, help="SteelProfile size (371 = the configuration the metric is quoted on)")
    ap.add_argument("--nsteps", type=int, default=45, help="Rosenbrock time steps per solve")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-general-path", action="store_true", help="skip the SteelProfile(5177) general-path leg (rank 0 at N = 1, n = 371 only)")
    ap.add_argument("--mode", choices=["replicas", "strong"], default="replicas",
                    help="replicas (default, weak scaling): one independent GDRE solve per GPU, K(t) gathered over RCCL; strong: ONE GDRE solve, the "
                         "same device-resident time loop on every rank; the independent shifted solves of a fan group are farmed over the ranks (rank r "
                         "takes the group positions s = r mod P and factorises only its shifts) with ONE in-place RCCL all-gather per GROUP; leftover "
                         "iterations are column-sharded; meant for --n 5177 / 20209 (BASELINE configs[3], [4])")
    ap.add_argument("--gather", choices=["lib", "torch"], default="lib",
                    help="replicas mode, N > 1: gather K(t) with the library's own communicator (dre_comm_allgather, default) or torch.distributed")
    ap.add_argument("--save-state", action="store_true", help="save_state=true (BASELINE configs[4]): every X(t) is kept, X stays factored")
    ap.add_argument("--cpu-steps", type=int, default=8, help="Rosenbrock time steps of the bounded CPU-baseline sample")
    ap.add_argument("--full", action="store_true",
                    help="after the headline record: roofline (one profiled solve), parity against the oracle's fixture, the other BASELINE configs "
                         "(rank 0 at N = 1, n = 371) and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write K(t) and the ADI iteration counts of the last timed solve as DIR/<name>.npy (rank 0)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


DUMP_BUDGET = 60 << 20          # bytes, all arrays of --dump-outputs together (under 64 MB with the .npy headers)


def dump_outputs(path, K, its):
    """K: (..., nt, m, n) float64 trajectories as a caller receives them (K(t_i) is m x n); its: ADI iterations per Lyapunov solve.  A K larger
    than the budget is cut to a fixed, seeded sample of its n columns (indices in K_columns.npy)."""
    os.makedirs(path, exist_ok=True)
    if os.path.abspath(path).startswith(ROOT + os.sep) and not os.path.exists(os.path.join(path, ".gitignore")):
        with open(os.path.join(path, ".gitignore"), "w") as f:          # benchmark outputs written inside the checkout stay out of git
            f.write("*\n")
    its = np.asarray(its, dtype=np.float64)
    n = K.shape[-1]
    col_bytes = K.nbytes // n
    room = (DUMP_BUDGET - its.nbytes) // (col_bytes + 8)
    if room < n:
        cols = np.sort(np.random.default_rng(0).choice(n, size=room, replace=False))
        K = K[..., cols]
        np.save(os.path.join(path, "K_columns.npy"), cols.astype(np.float64))
    np.save(os.path.join(path, "K.npy"), np.ascontiguousarray(K, dtype=np.float64))
    np.save(os.path.join(path, "adi_iterations.npy"), its)


def roofline_record(stats, n, m, pencil, its_solve, kw, wall):
    """Dominant kernel class (largest share of device time over BOTH streams of the context; dre_prof_* merges the side context) with its
    algorithmic bytes / flops per launch over the HIP-event time per launch, plus the whole solve against SURVEY 8(d) B_iter."""
    if not stats:
        return None
    stats = {k: dict(v) for k, v in stats.items()}
    if "mf_solve_real" in stats and "gemm_mf_top" in stats:
        # one shifted solve = level sweeps + gather + the dense top of the elimination tree (z-batched GEMM + slab reduction, class "gemm_mf_top"):
        # the algorithmic bytes of the scope cover the WHOLE solve, so its time must too
        top = stats.pop("gemm_mf_top")
        stats["mf_solve_real"]["ms"] += top["ms"]; stats["mf_solve_real"]["flops"] += top["flops"]
    name, s = max(stats.items(), key=lambda kv: kv[1]["ms"])
    total_ms = sum(v["ms"] for v in stats.values())
    avg_s = s["ms"] * 1e-3 / max(s["launches"], 1)
    if s["flops"] > 0 and s["bytes"] > 0 and s["flops"] / s["bytes"] > 12.0:
        ach = s["flops"] / max(s["launches"], 1) / avg_s / 1e12
        roof = dict(bound="mfma", kernel=name, achieved=ach, peak=78.6, unit="TFLOP/s", frac=ach / 78.6, traffic=None)
    else:
        ach = s["bytes"] / max(s["launches"], 1) / avg_s / 1e9
        roof = dict(bound="hbm", kernel=name, achieved=ach, peak=8000.0, unit="GB/s", frac=ach / 8000.0, traffic=None)
    roof["algorithmic_bytes_per_launch"] = s["bytes"] / max(s["launches"], 1)
    roof["algorithmic_flops_per_launch"] = s["flops"] / max(s["launches"], 1)
    for rnd in ("r05", "r04", "r03", "r02"):
        try:
            pmc_file = f"pmc_traffic_{rnd}_n{n}.json"
            pmc = json.load(open(os.path.join(ROOT, "profiles", pmc_file)))
            syms = SCOPE_SYMBOLS.get(name, [KERNEL_SYMBOL.get(name)])
            hits = [v for k, v in pmc["kernels"].items() if any(sy and sy in k for sy in syms)]
            if hits:
                tot_l = sum(h["launches"] for h in hits)
                run = pmc.get("run")
                if name == "mf_solve_real" and run:
                    roof["traffic"] = sum(h["fabric_bytes_per_launch"] * h["launches"] for h in hits) / max(run["solves"] * run["adi_iterations_per_solve"], 1)
                    roof["traffic_unit"] = "fabric bytes per shifted solve (all kernels of the scope: sweeps, top gather, dense top, slab reduction)"
                else:
                    roof["traffic"] = sum(h["fabric_bytes_per_launch"] * h["launches"] for h in hits) / max(tot_l, 1)
                    roof["traffic_unit"] = "fabric bytes per kernel launch"
                roof["traffic_source"] = (f"profiles/{pmc_file}: rocprofv3 --pmc FETCH_SIZE (x2 on gfx950) and WRITE_SIZE in separate passes; these are L2-fabric "
                                          "bytes, Infinity-Cache hits included (the working set of this size is MALL resident), not pure HBM bytes")
                break
        except Exception:
            pass
    roof.update(avg_launch_us=avg_s * 1e6, launches=s["launches"], share_of_device_time=s["ms"] / max(total_ms, 1e-12),
                measured_on="one extra profiled solve after the timed region (HIP events on the library's streams, main + side context merged)")
    roof["by_kernel_ms"] = {k: round(v["ms"], 3) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["ms"])[:8]}
    top_share = dict(roof)          # the class with the largest share of device time, whatever it is (kept for transparency)
    # the ADI iteration kernel itself (the hot op the metric counts), whatever class leads the device time: group chain (g iterations per
    # launch, n <= 768), single-iteration chain, or the multifrontal sweeps of the general path
    for cls in ("adi_group_iter", "adi_fast_iter", "mf_solve_real"):
        c = stats.get(cls)
        if c and c["launches"] > 0 and c["ms"] > 0:
            t = c["ms"] * 1e-3 / c["launches"]
            mf = c["flops"] > 0 and c["bytes"] > 0 and c["flops"] / c["bytes"] > 12.0
            ach = c["flops"] / c["launches"] / t / 1e12 if mf else c["bytes"] / c["launches"] / t / 1e9
            # SURVEY 8(d) defines the roofline figure per ADI ITERATION, so the record's headline entry is the ADI iteration kernel; when another
            # class leads the device time (n = 371: the Householder panel of the per-time-step residual compression) it is reported next to it
            if cls != name:
                roof.update(kernel=cls, bound="mfma" if mf else "hbm", achieved=ach, peak=78.6 if mf else 8000.0, unit="TFLOP/s" if mf else "GB/s",
                            frac=ach / (78.6 if mf else 8000.0), avg_launch_us=t * 1e6, launches=c["launches"], traffic=None,
                            algorithmic_flops_per_launch=c["flops"] / c["launches"], algorithmic_bytes_per_launch=c["bytes"] / c["launches"],
                            share_of_device_time=c["ms"] / max(total_ms, 1e-12))
                roof.pop("traffic_source", None)
                roof["largest_share_kernel"] = {k: top_share[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_us", "launches",
                                                                          "share_of_device_time", "algorithmic_bytes_per_launch", "algorithmic_flops_per_launch") if k in top_share}
                for rnd in ("r05", "r04", "r03", "r02"):
                    try:
                        pmc = json.load(open(os.path.join(ROOT, "profiles", f"pmc_traffic_{rnd}_n{n}.json")))
                        syms = SCOPE_SYMBOLS.get(cls, [KERNEL_SYMBOL.get(cls)])
                        hits = [v for k, v in pmc["kernels"].items() if any(sy and sy in k for sy in syms)]
                        if hits:
                            total = sum(h["fabric_bytes_per_launch"] * h["launches"] for h in hits)
                            run = pmc.get("run")
                            if cls == "mf_solve_real" and run:
                                # the SAME unit as algorithmic_bytes_per_launch (one shifted solve): everything the scope's kernels moved in the
                                # counter run over the shifted solves of that run (one per ADI iteration)
                                roof["traffic"] = total / max(run["solves"] * run["adi_iterations_per_solve"], 1)
                                roof["traffic_unit"] = "fabric bytes per shifted solve (all kernels of the scope: sweeps, top gather, dense top, slab reduction)"
                            else:
                                roof["traffic"] = total / max(sum(h["launches"] for h in hits), 1)
                                roof["traffic_unit"] = "fabric bytes per kernel launch"
                            roof["traffic_source"] = (f"profiles/pmc_traffic_{rnd}_n{n}.json: rocprofv3 --pmc FETCH_SIZE (x2 on gfx950) and WRITE_SIZE in separate passes; "
                                                      "L2-fabric bytes, Infinity-Cache hits included, not pure HBM bytes")
                            break
                    except Exception:
                        pass
            break
    # whole solve against the HBM roofline: SURVEY.md 8(d) B_iter per ADI iteration, summed with the measured residual widths
    pinfo = pencil.info()
    z, nnzF = float(pinfo["nnz"]), float(pinfo["factor_nnz"])
    kavg = kw / max(its_solve, 1.0)
    b_iter = 24.0 * z + 8.0 * n + 48.0 * n * kavg + 24.0 * n * m + 24.0 * nnzF + 32.0 * n * (kavg + m)
    ws = b_iter * its_solve / wall / 1e9
    roof["whole_solve"] = dict(bytes_per_iteration=b_iter, avg_residual_width=kavg, achieved=ws, unit="GB/s", peak=8000.0, frac=ws / 8000.0,
                               note="SURVEY.md 8(d) B_iter (algorithmic bytes of one real-shift ADI iteration) x ADI iterations / measured wall-clock of one solve")
    return roof


def parity_check(n, nsteps, Kdev_host, its):
    """K(t) of the solve that was just timed against the oracle's committed trajectory (tests/golden/make_fixtures_r03.py): delta of
    Stuff.jl:21 at the last time step (criterion of test/cuda.jl:95-99: < 1e-7) and the worst over all steps, plus the ADI iteration counts
    of every Lyapunov solve.  Fixtures exist for the metric's configuration (n = 371, 45 steps), n = 1357 (45 steps) and n = 5177 (12 steps)."""
    name = {(371, 45): "ros1_371_full", (1357, 45): "ros1_1357_full", (5177, 12): "ros1_5177_long", (5177, 45): "ros1_5177_full",
            (20209, 12): "ros1_20209_ss12"}.get((n, nsteps))
    if name is None:
        return None
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))

    def delta(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))
    K = [Kdev_host[i].T for i in range(nsteps + 1)]          # block i holds the m x n matrix K(t_i) column-major
    if "K" in g.files:
        ds = [delta(K[i], g["K"][i]) for i in range(1, nsteps + 1)]
    else:
        ds = [delta(K[i][:, ::16], g["K_cols"][i]) for i in range(1, nsteps + 1)]
    ref_its = [int(v) for v in g["iters"]]
    rec = dict(fixture=f"tests/golden/{name}.npz", delta_K_end=ds[-1], delta_K_worst=max(ds), criterion="delta < 1e-7 (test/cuda.jl:95-99)",
               iteration_counts_equal_oracle=bool(list(its) == ref_its), adi_iterations=int(sum(its)), adi_iterations_oracle=int(sum(ref_its)))
    # the metric's configuration must reproduce the oracle's count of EVERY Lyapunov solve; at n = 1357 one borderline decision at the steady
    # state (step 43: 1 iteration in the oracle, 0 on the device) is tolerated, as in tests/test_gpu_r03_full_length.py
    counts_ok = rec["iteration_counts_equal_oracle"] or (n != 371 and max(abs(a - b) for a, b in zip(its, ref_its)) <= 1)
    if not (rec["delta_K_worst"] < 1e-7 and counts_ok and len(its) == len(ref_its)):
        raise SystemExit(f"bench.py: PARITY FAILURE against {name}: {rec}")
    return rec


def general_path(D, ctx, args, n=5177, nsteps=12, steps=3, warmup=1, save_state=False, config=None):
    """The general sparse path (multifrontal sweeps, factored X, residual recurrence, sketch compression — everything the n <= 1536 dense special
    case is not), measured in the same run: SteelProfile(n) Ros1 LRSIF, Cyclic real shifts; parity against the oracle's fixture of that length.
    `setup_ms` = dre_pencil_create (nested-dissection ordering + symbolic analysis + upload; the reference pays its analysis inside every
    factorize call, blocklinear/backslash.jl:13), `first_solve_ms` = the cold solve (the ten numeric factorisations, top inverses, pool growth)."""
    import torch
    lib = ctx.lib
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    shifts = np.load(os.path.join(ROOT, "tests", "golden", f"heuristic_shifts_{n}.npy"))
    ctx.sync(); tsu = time.perf_counter()
    pencil = D.Pencil(d.E, d.A, ctx)
    ctx.sync(); setup_ms = (time.perf_counter() - tsu) * 1e3
    Bd, Cd = ctx.upload(d.B), ctx.upload(d.C)
    X0 = D.DeviceLDLt.create(ctx, pencil, L, Dm, 1.0)
    opt, keep = D.device.make_adi_options(shift_kind=0, shifts=list(shifts), maxiters=200)
    m = d.B.shape[1]
    Kdev = torch.empty((nsteps + 1, n, m), dtype=torch.float64, device="cuda")
    t0, dt = 4500.0, -100.0
    rec = {}

    def one():
        r = C.c_void_p()
        ctx.chk(lib.dre_gdre_solve(ctx.ptr, pencil.ptr, Bd.ptr, Cd.ptr, X0.ptr, t0, t0 + dt * nsteps, dt, 1, 1 if save_state else 0, C.byref(opt), C.byref(r)))
        ii = (C.c_int64 * 7)()
        lib.dre_gdre_result_info(r, ii)
        ctx.chk(lib.dre_gdre_result_K_device(ctx.ptr, r, C.c_void_p(Kdev.data_ptr())))
        its, kw = [], 0.0
        for j in range(ii[4]):
            gi = (C.c_int64 * 4)(); gd = (C.c_double * 2)()
            lib.dre_gdre_result_gale(r, j, gi, gd)
            its.append(int(gi[0])); kw += float(gi[0]) * float(gi[3])
        if save_state:
            # storage of the trajectory X(t): every stored state as factors L (n x r) and D (r x r)
            xb, ranks = 0, []
            for j in range(ii[1]):
                xp = C.c_void_p(); nn = C.c_int(); rr = C.c_int(); nb = C.c_int()
                lib.dre_gdre_result_X(r, j, C.byref(xp))
                lib.dre_ldlt_info(xp, C.byref(nn), C.byref(rr), C.byref(nb))
                ranks.append(int(rr.value)); xb += 8 * (int(nn.value) * int(rr.value) + int(rr.value) ** 2)
            rec.update(x_storage_bytes=xb, x_ranks=ranks)
        lib.dre_gdre_result_free(r)
        rec.update(its=its, kw=kw, nfac=int(ii[3]))
        return int(ii[2])
    ctx.sync(); tf = time.perf_counter()
    one()
    ctx.sync(); first_ms = (time.perf_counter() - tf) * 1e3
    for _ in range(max(warmup - 1, 0)):
        one()
    ctx.sync(); torch.cuda.synchronize()
    ts = time.perf_counter()
    iters = sum(one() for _ in range(steps))
    ctx.sync(); torch.cuda.synchronize()
    el = time.perf_counter() - ts
    ctx.prof_reset(); ctx.prof_enable(True)
    one()
    stats = ctx.prof_stats()
    ctx.prof_enable(False)
    roof = roofline_record(stats, n, m, pencil, iters / steps, rec["kw"], el / steps)
    par = parity_check(n, nsteps, Kdev.cpu().numpy(), rec["its"])
    return dict(config=config,
                workload=f"SteelProfile({n}) surrogate, Ros1 LRSIF, Cyclic real shifts, {nsteps} time steps (tspan=(4500,{t0 + dt * nsteps:g}), dt=-100)"
                         f"{', save_state=true' if save_state else ''}: batched multifrontal fan groups + residual recurrence + side-stream compression of X",
                n=n, nsteps=nsteps, steps=steps, warmup=warmup, save_state=bool(save_state),
                value=iters / el, unit="ADI iterations/s", ms_per_step=el / steps * 1e3, adi_iterations_per_solve=iters / steps,
                setup_ms=setup_ms, first_solve_ms=first_ms,
                sparse_factorizations_per_solve=rec["nfac"], roofline=roof, parity=par,
                **({"x_storage_bytes": rec["x_storage_bytes"], "x_rank_min_max": [min(rec["x_ranks"][1:] or [0]), max(rec["x_ranks"])],
                    "stored_states": len(rec["x_ranks"])} if save_state else {}))


def ros2_projection_leg(D, ctx, steps=2):
    """BASELINE configs[2] as written: SteelProfile(1357) Ros2 LRSIF with the DEFAULT ADI() = Projection(2) shifts (complex pairs on the
    non-symmetric surrogate variant), 10 steps of dt = -20; parity against tests/golden/ros2_1357_proj.npz (the oracle's K(t) where the oracle
    converges, the dense Ros2 solver's K(t) everywhere)."""
    import warnings
    g = np.load(os.path.join(ROOT, "tests", "golden", "ros2_1357_proj.npz"))
    n = 1357
    d = D.steel_profile(n, convection=float(g["convection"]))
    L, Dm = D.initial_value(d)
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4300.0))
    alg = D.Ros2(D.ADI(maxiters=200))
    warnings.simplefilter("ignore")
    D.set_default_context(ctx)
    ctx.sync(); t = time.perf_counter()
    sol, st = D.solve_gdre(prob, alg, dt=float(g["dt"]), return_stats=True, ctx=ctx)
    first_ms = (time.perf_counter() - t) * 1e3
    els = []
    for _ in range(steps):
        ctx.sync(); t = time.perf_counter()
        sol, st = D.solve_gdre(prob, alg, dt=float(g["dt"]), return_stats=True, ctx=ctx)
        els.append(time.perf_counter() - t)
    best = sum(els) / len(els)            # the MEAN of the timed runs (the leg reported the better of two)
    ctx.prof_reset(); ctx.prof_enable(True)
    D.solve_gdre(prob, alg, dt=float(g["dt"]), ctx=ctx)
    stats = ctx.prof_stats(); ctx.prof_enable(False)

    def delta(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b)))
    its = [x["iters"] for x in st["gales"]]
    ncx = sum(int(np.sum(np.abs(np.imag(x["shifts"])) > 0)) for x in st["gales"])
    par = dict(fixture="tests/golden/ros2_1357_proj.npz", delta_K_vs_oracle_steps_1_8=max(delta(sol.K[i], g["K"][i]) for i in range(1, 9)),
               delta_K_vs_dense_ros2_worst=max(delta(sol.K[i], g["K_dense"][i]) for i in range(1, 11)),
               adi_iterations=int(sum(its)), adi_iterations_oracle=int(g["iters_per_solve"].sum()),
               lyapunov_solves_converged=f"{sum(int(x['converged']) for x in st['gales'])}/{len(its)}", oracle_solves_converged=f"{int((~g['failed']).sum())}/{len(g['failed'])}",
               complex_shift_share=ncx / max(sum(its), 1), adi_iterations_per_solve=its, adi_iterations_per_solve_oracle=[int(v) for v in g["iters_per_solve"]],
               residual_widths_per_solve=[int(x["rhs_cols"]) for x in st["gales"]], criterion="delta < 1e-7 where the oracle converges (test/cuda.jl:95-99); counts within a Projection batch")
    if not (par["delta_K_vs_oracle_steps_1_8"] < 1e-7 and par["delta_K_vs_dense_ros2_worst"] < 1e-6):
        raise SystemExit(f"bench.py: PARITY FAILURE (configs[2]): {par}")
    tot = sum(v["ms"] for v in stats.values())
    name, sk = max(stats.items(), key=lambda kv: kv[1]["ms"])
    avg_s = sk["ms"] * 1e-3 / max(sk["launches"], 1)
    roof = dict(bound="hbm", kernel=name, achieved=sk["bytes"] / max(sk["launches"], 1) / max(avg_s, 1e-12) / 1e9, peak=8000.0, unit="GB/s", traffic=None,
                avg_launch_us=avg_s * 1e6, launches=sk["launches"], share_of_device_time=sk["ms"] / max(tot, 1e-12),
                by_kernel_ms={k: round(v["ms"], 3) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["ms"])[:8]})
    roof["frac"] = roof["achieved"] / 8000.0
    return dict(config="BASELINE configs[2]", workload="SteelProfile(1357) surrogate + convection (non-symmetric), Ros2 LRSIF, default ADI() = Projection(2) shifts "
                "(complex pairs), 10 time steps of dt=-20, 20 Lyapunov solves", n=n, nsteps=10, value=sum(its) / best, unit="ADI iterations/s",
                value_normalised_to_oracle_iterations=float(g["iters_per_solve"].sum()) / best,
                ms_per_step=best * 1e3, ms_per_step_runs=[round(e * 1e3, 2) for e in els], first_solve_ms=first_ms, adi_iterations_per_solve=sum(its),
                roofline=roof, parity=par)


def ros2_general_leg(D, ctx, steps=2):
    """Ros2 on the GENERAL path (/root/reference/src/riccati/lowrank_ros2.jl:37-80): SteelProfile(5177) Ros2 LRSIF, Cyclic
    real shifts, 12 steps of dt = -100 — two cold-start Lyapunov solves per step, fan groups on both.  The shift list is the heuristic list of
    (E, A) mapped like the spectrum of the Ros2 operator F = gamma tau A - E / 2 - ... (lowrank_ros2.jl:41: gamma tau lambda - 1/2), so that every
    stage solve converges (29 - 47 iterations; with the unmapped list none does within maxiters = 200: that case stays a test,
    tests/test_gpu_r05.py).  Parity against tests/golden/ros2_5177_conv.npz (oracle/dre_oracle.py): K(t) to 1e-7, the iteration count of every
    stage solve within one of the oracle's."""
    import warnings
    g = np.load(os.path.join(ROOT, "tests", "golden", "ros2_5177_conv.npz"))
    n, nsteps = 5177, 12
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4500.0 - 100.0 * nsteps))
    alg = D.Ros2(D.ADI(shifts=D.Shifts.Cyclic(list(g["shifts"])), maxiters=200))
    warnings.simplefilter("ignore")
    D.set_default_context(ctx)
    sol, st = D.solve_gdre(prob, alg, dt=-100.0, return_stats=True, ctx=ctx)
    els = []
    for _ in range(steps):
        ctx.sync(); t = time.perf_counter()
        sol, st = D.solve_gdre(prob, alg, dt=-100.0, return_stats=True, ctx=ctx)
        els.append(time.perf_counter() - t)
    mean = sum(els) / len(els)
    ctx.prof_reset(); ctx.prof_enable(True)
    D.solve_gdre(prob, alg, dt=-100.0, ctx=ctx)
    stats = ctx.prof_stats(); ctx.prof_enable(False)
    its = [x["iters"] for x in st["gales"]]
    ref = [int(v) for v in g["iters_per_solve"].ravel()]
    w = np.random.default_rng(1).standard_normal(n)
    dk = max(float(np.linalg.norm(sol.K[i][:, ::16] - g["K_cols"][i]) / g["K_norm"][i]) for i in range(1, nsteps + 1))
    dw = max(float(np.linalg.norm(sol.K[i] @ w - g["K_w"][i]) / np.linalg.norm(g["K_w"][i])) for i in range(1, nsteps + 1))
    nconv = sum(int(x["converged"]) for x in st["gales"])
    par = dict(fixture="tests/golden/ros2_5177_conv.npz", delta_K_sampled_columns=dk, delta_K_times_seeded_vector=dw, adi_iterations_per_solve=its,
               adi_iterations_per_solve_oracle=ref, lyapunov_solves_converged=f"{nconv}/{len(its)}", oracle_solves_converged=f"{sum(int(v < 200) for v in ref)}/{len(ref)}",
               criterion="delta < 1e-7 (test/cuda.jl:95-99), every stage solve converged, its iteration count within one of the oracle's")
    if not (dk < 1e-7 and dw < 1e-7 and nconv == len(its) and all(abs(a - b) <= 1 for a, b in zip(its, ref))):
        raise SystemExit(f"bench.py: PARITY FAILURE (Ros2, general path): {par}")
    tot = sum(v["ms"] for v in stats.values())
    return dict(config="SURVEY 8(a) a2 on the general path (no BASELINE config of its own)", workload="SteelProfile(5177) Ros2 LRSIF, Cyclic real shifts (the heuristic "
                "list mapped to the Ros2 operator), 12 time steps of dt=-100, 24 cold-start Lyapunov solves, all converged",
                n=n, nsteps=nsteps, value=sum(its) / mean, unit="ADI iterations/s", value_normalised_to_oracle_iterations=sum(ref) / mean,
                ms_per_step=mean * 1e3, ms_per_step_runs=[e * 1e3 for e in els],
                parity=par, by_kernel_ms={k: round(v["ms"], 3) for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["ms"])[:8]}, device_ms_profiled=tot)


def launch_ranks(args):
    """`python bench.py --gpus N` without a torchrun environment: start the N ranks ourselves (fresh child processes under
    torch.distributed.run, BEFORE anything in this process touches the GPU) and relay rank 0's JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.run(cmd, env=env)
    raise SystemExit(proc.returncode)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        launch_ranks(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} (or without torchrun)")
    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the engine has no CPU fallback")
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    import dre_amd as D
    from dre_amd.replicas import gather_trajectories, reduce_timing

    n = args.n
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    shifts = np.load(os.path.join(ROOT, "tests", "golden", f"heuristic_shifts_{n}.npy"))
    t0, dt = 4500.0, -100.0
    tf = t0 + dt * args.nsteps

    ctx = D.Context(local_rank)
    lib = ctx.lib
    ctx.sync(); t_su = time.perf_counter()
    pencil = D.Pencil(d.E, d.A, ctx)
    ctx.sync(); setup_ms = (time.perf_counter() - t_su) * 1e3       # dre_pencil_create: ordering + symbolic analysis + upload (outside the timed region)
    strong = args.mode == "strong"
    # The communicator lives INSIDE the library (RCCL over xGMI on the library stream).  replicas: it gathers the K(t) trajectories;
    # strong: it carries the one all-gather of V per ADI step of the column-sharded solve.  torch.distributed only hands the unique id around.
    from dre_amd.replicas import attach_communicator
    use_lib_comm = strong or (world > 1 and args.gather == "lib")
    comm_note = None
    if use_lib_comm:
        try:
            attach_communicator(ctx, rank, world)
        except Exception as e:          # replicas: the gather of K(t) is auxiliary — fall back to torch.distributed and SAY so; strong mode has no fallback
            if strong:
                raise
            comm_note = f"library communicator failed on rank {rank} ({e}); K(t) gathered by torch.distributed"
            print(f"[bench] {comm_note}", file=sys.stderr, flush=True)
            use_lib_comm = False
        if world > 1 and not strong:
            # every rank must take the same path: if any rank fell back, all do
            flag = torch.tensor([1.0 if use_lib_comm else 0.0], device="cuda")
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if float(flag.item()) == 0.0 and use_lib_comm:
                ctx.comm_free(); use_lib_comm = False
                comm_note = "another rank's library communicator failed; K(t) gathered by torch.distributed"
        if use_lib_comm and not strong:
            ctx.set_option("shard_min_cols", 1 << 30)        # replicas: the communicator only gathers K(t), every rank solves its own problem
    # replicas: rank r starts from a slightly different X0 (0.01 * (1 + r/8) * L L'); strong: the SAME problem on every rank
    Bd, Cd = ctx.upload(d.B), ctx.upload(d.C)
    X0 = D.DeviceLDLt.create(ctx, pencil, L, Dm * (1.0 if strong else 1.0 + rank / 8.0), 1.0)
    opt, keep = D.device.make_adi_options(shift_kind=0, shifts=list(shifts), maxiters=100 if n <= 371 else 200)
    m = d.B.shape[1]
    nt = args.nsteps + 1
    Kdev = torch.empty((nt, n, m), dtype=torch.float64, device="cuda")       # nt blocks of m x n column-major
    Kall = torch.empty((world, nt, n, m), dtype=torch.float64, device="cuda") if (world > 1 and not strong) else None

    width = {"kw": 0.0}

    def one_solve(gather=True):
        r = C.c_void_p()
        ctx.chk(lib.dre_gdre_solve(ctx.ptr, pencil.ptr, Bd.ptr, Cd.ptr, X0.ptr, t0, tf, dt, 1, 1 if args.save_state else 0, C.byref(opt), C.byref(r)))
        ii = (C.c_int64 * 7)()
        lib.dre_gdre_result_info(r, ii)
        ctx.chk(lib.dre_gdre_result_K_device(ctx.ptr, r, C.c_void_p(Kdev.data_ptr())))
        ngale = ii[4]
        nconv = 0
        kw = 0.0                      # sum over Lyapunov solves of iterations x residual width (for the whole-solve byte count)
        its = []
        for j in range(ngale):
            gi = (C.c_int64 * 4)(); gd = (C.c_double * 2)()
            lib.dre_gdre_result_gale(r, j, gi, gd)
            nconv += int(gi[1])
            kw += float(gi[0]) * float(gi[3])
            its.append(int(gi[0]))
        width["kw"] = kw; width["its"] = its
        lib.dre_gdre_result_free(r)
        if Kall is not None and gather:
            gather_trajectories(ctx if use_lib_comm else None, Kdev, Kall, world)     # RCCL over xGMI: the K(t) trajectories of all replicas
        return int(ii[2]), int(ii[3]), nconv, ngale

    def barrier():
        ctx.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    ctx.sync(); t_first = time.perf_counter()
    if args.warmup > 0:
        one_solve()
    ctx.sync(); first_solve_ms = (time.perf_counter() - t_first) * 1e3 if args.warmup > 0 else None      # cold: factorisations, stacks, pool growth, rank hints
    for _ in range(args.warmup - 1):
        one_solve()
    barrier()
    t_start = time.perf_counter()
    iters = 0
    for _ in range(args.steps):
        it, nfac, nconv, ngale = one_solve()
        iters += it
    barrier()
    elapsed = time.perf_counter() - t_start
    elapsed, total_iters = reduce_timing(elapsed, float(iters), torch.device('cuda', local_rank), world)
    if strong:
        total_iters /= world          # ONE problem: every rank counted the same iterations

    out = None
    parity_failure = None
    its_last = list(width["its"])
    if rank == 0 and args.dump_outputs:
        # what the last timed solve returned: K(t_i) as m x n matrices (block i of Kdev is m x n column-major), per replica when gathered
        dump_outputs(args.dump_outputs, (Kall if Kall is not None else Kdev).transpose(-1, -2).cpu().numpy(), its_last)
    if args.full and strong and world > 1 and rank != 0:
        one_solve(gather=False)      # strong mode: every ADI group enqueues a collective, so the profiled extra solve of rank 0 needs its partners
    if rank == 0:
        if args.full:
            # ---- roofline leg: one extra identical solve with per-kernel HIP-event timing on the library stream
            ctx.prof_reset()
            ctx.prof_enable(True)
            one_solve(gather=False)      # replicas: the profiled solve does not gather (collectives stay matched); strong: all ranks run it (above)
            stats = ctx.prof_stats()
            ctx.prof_enable(False)
            if os.environ.get("DRE_BENCH_CLASSES"):        # builder's view: every kernel class of the profiled solve (stderr; the JSON line is unchanged)
                for k_, v_ in sorted(stats.items(), key=lambda kv: -kv[1]["ms"]):
                    print(f"[class] {k_:24s} launches {v_['launches']:6d}  ms {v_['ms']:9.3f}  avg_us {v_['ms'] * 1e3 / max(v_['launches'], 1):8.2f}", file=sys.stderr)
            roof = roofline_record(stats, n, m, pencil, total_iters / (args.steps * (1 if strong else world)), width["kw"], elapsed / args.steps)
            # ---- parity leg (after the timed region): the K(t) trajectory of the last timed solve of rank 0 against the committed oracle fixture
            try:
                parity = parity_check(n, args.nsteps, Kdev.cpu().numpy(), its_last)
            except SystemExit as e:      # reported AFTER the final barrier: a parity failure must not strand the other ranks in it
                parity, parity_failure = None, e
            # ---- general path leg: the sparse multifrontal path north_star names, in the driver-timed record
            general = general45 = general20k = general20k45 = ros2leg = ros2gen = None
            if world == 1 and n == 371 and not strong and not args.no_general_path:
                general = general_path(D, ctx, args, config="BASELINE configs[3], first 12 of its 45 steps (the leg of rounds 2-3)")
                general45 = general_path(D, ctx, args, nsteps=45, steps=2, warmup=1, config="BASELINE configs[3] at its stated length (one GPU)")
                general20k = general_path(D, ctx, args, n=20209, nsteps=12, steps=2, warmup=1, save_state=True, config="BASELINE configs[4] (one GPU), 12 of 45 steps")
                general20k45 = general_path(D, ctx, args, n=20209, nsteps=45, steps=1, warmup=1, save_state=True,
                                            config="BASELINE configs[4] at its stated length (one GPU): 45 steps, save_state; no oracle fixture of this length "
                                                   "(the 12-step one took the oracle 26 minutes) - tests/test_gpu_r05.py checks it through size-independent properties")
                ros2leg = ros2_projection_leg(D, ctx)
                ros2gen = ros2_general_leg(D, ctx)
            # ---- CPU baseline leg: the oracle (a NumPy/SciPy port with the reference's algorithmic choices) on a bounded sample.
            # The BLAS thread count matters a lot at this size (128 OpenBLAS threads are 13x SLOWER than one on 371-row panels),
            # so a two-step probe picks the fastest of a few thread counts and the sample runs with that one.
            cpu = None
            if not args.no_cpu_baseline and world == 1:       # rank 0 at N = 1 only
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import warnings
                import dre_oracle as o
                from threadpoolctl import threadpool_limits
                warnings.simplefilter("ignore")

                def cpu_run(nsteps_cpu, threads, reuse=False):
                    st = []
                    with threadpool_limits(limits=threads):
                        tc = time.perf_counter()
                        o.solve(o.GDREProblem(d.E, d.A, d.B, d.C, o.lowrank(L, Dm), (t0, t0 + dt * nsteps_cpu)),
                                o.Ros1(o.ADI(shifts=o.Cyclic(list(shifts)), factor_cache=o.FactorCache(reuse=reuse))), dt=dt, stats=st)
                        tc = time.perf_counter() - tc
                    return sum(x["iters"] for x in st), tc

                ncpu = os.cpu_count() or 1
                probe = {}
                big = n > 1500            # one Rosenbrock step of the oracle takes tens of seconds there: the probe IS the sample
                for th in (sorted({1, 4, min(16, ncpu)}) if not big else [min(16, ncpu)]):
                    print(f"[bench] cpu baseline: probing {th} BLAS thread(s)", file=sys.stderr, flush=True)
                    it_p, t_p = cpu_run(min(args.nsteps, 2), th)
                    probe[th] = it_p / t_p
                    if big: cpu_it, tc, nsteps_cpu = it_p, t_p, min(args.nsteps, 2)
                best = max(probe, key=probe.get)
                fair = None
                if not big:
                    # bounded sample: the full 45-step workload if the probe says it fits ~30 s, else args.cpu_steps steps
                    est_full = 746.0 / probe[best] * (n / 371.0) ** 2
                    nsteps_cpu = args.nsteps if est_full < 30.0 else args.cpu_steps
                    print(f"[bench] cpu baseline: {nsteps_cpu} steps with {best} thread(s)", file=sys.stderr, flush=True)
                    cpu_it, tc = cpu_run(nsteps_cpu, best)
                    it2, tc2 = cpu_run(nsteps_cpu, best, reuse=True)
                    fair = dict(value=it2 / tc2, unit="ADI iterations/s",
                                note="same sample and threads, sparse LU factors reused per shift like the engine (the reference refactorises every ADI step)")
                # BASELINE configs[0]: the DENSE Rosenbrock-1 solver on the CPU (reference plumbing, src/riccati/dense_ros1.jl:30-49), a bounded sample
                dense0 = None
                if n <= 400:
                    with threadpool_limits(limits=best):
                        td = time.perf_counter()
                        o.solve(o.GDREProblem(d.E, d.A, d.B, d.C, o.lowrank(L, Dm).dense(), (t0, t0 + dt * 5)), o.Ros1(), dt=dt)
                        td = time.perf_counter() - td
                    dense0 = dict(config="BASELINE configs[0]", workload=f"SteelProfile({n}) dense Ros1 on the CPU (oracle), 5 of 45 time steps", s_per_time_step=td / 5.0,
                                  threads=best)
                cpu = dict(value=cpu_it / tc, unit="ADI iterations/s", cores=best, kind="port", factor_caching_variant=fair, dense_ros1_config0=dense0,
                           thread_probe_it_per_s={str(k): round(v, 1) for k, v in probe.items()},
                           sample=f"{nsteps_cpu} of {args.nsteps} Rosenbrock steps of the same workload ({cpu_it} ADI iterations, {tc:.1f} s), "
                                  f"NumPy/SciPy oracle with {best} BLAS thread(s) ({'fastest of the probed counts' if not big else 'single probe at this size'}; {ncpu} host CPUs), "
                                  f"SuperLU refactorised every ADI step like the reference")
        out = {
            "metric": "ADI iterations/sec (GDRE Ros1 LRSIF, SteelProfile surrogate)",
            "value": total_iters / elapsed,
            "unit": "ADI iterations/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "gdre_wall_clock_s": elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"SteelProfile({n}) surrogate, Ros1 LRSIF (LDL' X0), Cyclic real shifts (10 heuristic values), "
                                   f"tspan=(4500,{tf:g}), dt=-100, {args.nsteps} time steps",
                       "adi_iterations_per_solve": total_iters / (args.steps * (1 if strong else world)),
                       "lyapunov_solves_converged": f"{nconv}/{ngale}",
                       "sparse_factorizations_per_solve": nfac,
                       "save_state": bool(args.save_state),
                       "parallelism": (f"ONE solve, fan groups shift-sharded x{world} inside the library (one RCCL all-gather per group of up to 8 ADI iterations)" if strong else
                                       f"replicas x{world}" + ((" + K(t) gathered by " + ("dre_comm_allgather (RCCL inside the library)" if use_lib_comm
                                                                                          else "torch.distributed all_gather")) if world > 1 else "")),
                       "comm": ctx.comm_info() if use_lib_comm else comm_note},
        }
        if args.full:
            out["config"]["parity"] = parity
            out.update(roofline=roof, cpu_baseline=cpu, general_path=general, general_path_45=general45, general_path_20209=general20k,
                       general_path_20209_45=general20k45, ros2_1357_projection=ros2leg, ros2_general_5177=ros2gen)
        out["setup_ms"] = setup_ms
        out["first_solve_ms"] = first_solve_ms
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if parity_failure is not None:
        raise parity_failure
    if rank == 0:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
