"""final_x_lazy = 0 / 1 alternated solve by solve in ONE process (no process-to-process noise): the headline solve as bench.py times it
(dre_gdre_solve + K(t) export + per-solve records + free; the final X is never requested).  usage: ab_final_x.py [pairs] [n] [nsteps]"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import dre_amd as D

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 100
n = int(sys.argv[2]) if len(sys.argv) > 2 else 371
nsteps = int(sys.argv[3]) if len(sys.argv) > 3 else 45
d = D.steel_profile(n); L, Dm = D.initial_value(d)
ctx = D.Context(0); lib = ctx.lib
pencil = D.Pencil(d.E, d.A, ctx)
Bd, Cd = ctx.upload(d.B), ctx.upload(d.C)
X0 = D.DeviceLDLt.create(ctx, pencil, L, Dm, 1.0)
shifts = list(np.load(os.path.join(ROOT, "tests", "golden", f"heuristic_shifts_{n}.npy")))
opt, keep = D.device.make_adi_options(shift_kind=0, shifts=shifts, maxiters=100 if n <= 371 else 200)
Kdev = torch.empty((nsteps + 1, n, d.B.shape[1]), dtype=torch.float64, device="cuda")


def one():
    r = C.c_void_p()
    ctx.chk(lib.dre_gdre_solve(ctx.ptr, pencil.ptr, Bd.ptr, Cd.ptr, X0.ptr, 4500.0, 4500.0 - 100.0 * nsteps, -100.0, 1, 0, C.byref(opt), C.byref(r)))
    ii = (C.c_int64 * 7)()
    lib.dre_gdre_result_info(r, ii)
    ctx.chk(lib.dre_gdre_result_K_device(ctx.ptr, r, C.c_void_p(Kdev.data_ptr())))
    for j in range(ii[4]):
        gi = (C.c_int64 * 4)(); gd = (C.c_double * 2)()
        lib.dre_gdre_result_gale(r, j, gi, gd)
    lib.dre_gdre_result_free(r)


for _ in range(6):
    one()
ts = {0: [], 1: []}
for p in range(pairs):
    for v in ((0, 1) if p % 2 == 0 else (1, 0)):
        ctx.set_option("final_x_lazy", v)
        ctx.sync(); t = time.perf_counter()
        one()
        ctx.sync(); ts[v].append((time.perf_counter() - t) * 1e3)
for v in (0, 1):
    a = np.sort(np.array(ts[v]))
    print(f"final_x_lazy={v}: {len(a)} solves, median {np.median(a):.3f} ms, quartiles {a[len(a) // 4]:.3f} .. {a[3 * len(a) // 4]:.3f}, min {a[0]:.3f}, max {a[-1]:.3f}")
dif = np.array(ts[0]) - np.array(ts[1])
print(f"paired difference (0 minus 1): median {np.median(dif):.3f} ms, quartiles {np.sort(dif)[len(dif) // 4]:.3f} .. {np.sort(dif)[3 * len(dif) // 4]:.3f}, "
      f"positive in {int((dif > 0).sum())} of {len(dif)} pairs")
