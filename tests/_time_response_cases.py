"""The systems, grids and signals of the time-response tests (tests/test_time_response_host.py, tests/test_gpu_time_response.py) and the record
tests/golden/time_response.json (arrays: tests/golden/time_response_ref.npz).

Cases (E x' = A x + B u, y = C x), the systems of tests/_freq_cases.py:
  scalar1        n = 1 (E = 2, A = -3), dt = 0.1, K = 40
  unstable1      n = 1, E = 1, A = 0.5: a growing response is a valid result; dt = 0.1, K = 40
  osc12          the lightly damped oscillator, dt = 0.02, K = 1000: rho(M) = 1 - 1e-7 under tustin, ||M||_2 = 2.7: the hard case for doubling
  index1_6       singular E: backward Euler only, step and simulate only; dt = 0.1, K = 60
  pencil33       dt = 0.05, K = 127 (the block-edge tests take its prefixes); pencil70, pencil33_m1, pencil33_q1: dt = 0.05, K = 64
  pencil371      dt = 0.05, K = 300; to keep the record below 1 MB it holds the tustin step response and simulate of both methods
Kinds per case and method: step, impulse (regular E), simulate with S = 2 scenarios (pencil33: 3; `signals`; scenario 0 starts from x_0 = 0).
The signals are dyadic rationals from an integer hash of (seed, s, k, c): the same bits on every machine, no random generator's stream.

The record holds per case, method and kind
  Y_ref       the sequential recurrence x_{k+1} = M x_k + N w_k with P^-1, M, N and the recurrence in mpmath at 50 digits (n <= 70), rounded
              to double once; at n = 371 P^-1 [E, B] from an LU solve refined four times with numpy.longdouble residuals and the recurrence in
              numpy.longdouble;
  model_dist  the distance of the NumPy model (_time_response_model.py, default block) to Y_ref; model_dist_L for L = 4, 64, 256;
  lapack_dist the distance of the plain float64 recurrence (_time_response_model.sequential) to Y_ref,
with the distance  max_k ||Y_k - Yref_k||_F / max_k ||Yref_k||_F  (simulate: per scenario).  Further:
  steady      pencil33 and pencil70 under tustin at dt = 4, K = 64 (rho(M)^64 recorded, below 1e-17): the last sample of the step response,
              whose limit is the static gain -C A^-1 B exactly (tustin's fixed point), with the model's distance for it;
  order       the exact step response of pencil33 on t = 0.1 i, i = 0 .. 64, from scipy.linalg.expm (zero-order hold, exact for a step), and
              the NumPy model's error ratios under halving dt = 0.1, 0.05, 0.025.
The arrays (Y_ref, the steady samples, the exact step response) are float64 in tests/golden/time_response_ref.npz under the keys that the
JSON names; the JSON holds the grids, the distances and everything else.
Regenerate with:  python tests/_time_response_cases.py   (needs mpmath and scipy; the tests read only the JSON)."""
import functools
import json
import os

import numpy as np

import _freq_cases as fc
import _time_response_model as tm

HERE = os.path.dirname(os.path.abspath(__file__))
DPS = 50
REFINE_STEPS = 4
METHODS = tm.METHODS
KINDS = ("step", "impulse", "simulate")
S_REC = {"pencil33": 3}        # scenarios of simulate in the record; 2 elsewhere
GRID = {   # name: (dt, K)
    "scalar1": (0.1, 40), "unstable1": (0.1, 40), "osc12": (0.02, 1000), "index1_6": (0.1, 60), "pencil33": (0.05, 127), "pencil70": (0.05, 64),
    "pencil33_m1": (0.05, 64), "pencil33_q1": (0.05, 64), "pencil371": (0.05, 300),
}
CASES = tuple(GRID)
STEADY = {"pencil33": (4.0, 64), "pencil70": (4.0, 64)}
ORDER_CASE, ORDER_T, ORDER_DTS = "pencil33", 6.4, (0.1, 0.05, 0.025)
MODEL_BLOCKS = (4, 64, 256)


def record_path():
    return os.path.join(HERE, "golden", "time_response.json")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


def arrays_path():
    return os.path.join(HERE, "golden", "time_response_ref.npz")


@functools.lru_cache(maxsize=None)
def arrays():
    with np.load(arrays_path()) as z:
        return {k: z[k] for k in z.files}


_NEW_ARRAYS = {}        # filled by build_record


def enc(a, key):
    """keep the array for the .npz, name it in the JSON"""
    _NEW_ARRAYS[key] = np.ascontiguousarray(a, dtype=float)
    return dict(npz=key, shape=list(np.shape(a)))


def dec(d):
    a = arrays()[d["npz"]]
    assert list(a.shape) == d["shape"]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def system(name):
    """(E, A, B, C), read-only"""
    if name == "unstable1":
        mats = (np.array([[1.0]]), np.array([[0.5]]), np.array([[1.5]]), np.array([[0.7]]))
        for M in mats:
            M.setflags(write=False)
        return mats
    return fc.system(name)


def present(name):
    """the (method, kind) pairs of a case in the record"""
    if name == "index1_6":
        return [("backward_euler", "step"), ("backward_euler", "simulate")]
    if name == "pencil371":
        return [("tustin", "step"), ("tustin", "simulate"), ("backward_euler", "simulate")]
    return [(me, ki) for me in METHODS for ki in KINDS]


ALL = tuple((name, me, ki) for name in CASES for me, ki in present(name))


def _hash01(seed, s, k, c):
    """a dyadic rational in [-1, 1) from an integer hash: exact in float64"""
    x = (seed * 1000003 + s * 1299709 + k * 7919 + c * 104729 + 12345) & 0xFFFFFFFF
    x = (x * 2654435761) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 2246822519) & 0xFFFFFFFF
    x ^= x >> 13
    return (x >> 8) / float(1 << 23) - 1.0


@functools.lru_cache(maxsize=None)
def signals(name):
    """(u (S, K+1, m), x0 (S, n)); scenario 0 starts from x_0 = 0"""
    S = S_REC.get(name, 2)
    _, K = GRID[name]
    E, _, B, _ = system(name)
    n, m = B.shape
    seed = CASES.index(name) + 1
    u = np.array([[[_hash01(seed, s, k, c) for c in range(m)] for k in range(K + 1)] for s in range(S)])
    x0 = np.array([[0.0 if s == 0 else _hash01(seed + 100, s, i, 0) for i in range(n)] for s in range(S)])
    u.setflags(write=False)
    x0.setflags(write=False)
    return u, x0


def recorded_case(name, method, kind):
    """(Y_ref, model_dist, lapack_dist): step, impulse (K+1, q, m) and scalars; simulate (S, K+1, q) and arrays of S"""
    r = recorded()["cases"][name][method][kind]
    return dec(r["Y_ref"]), np.asarray(r["model_dist"], dtype=float), np.asarray(r["lapack_dist"], dtype=float)


def bound(name, method, kind):
    """the device bound: max(10 x max(model's, LAPACK's recorded distance), 2 n eps)"""
    _, md, ld = recorded_case(name, method, kind)
    n = system(name)[0].shape[0]
    return np.maximum(10.0 * np.maximum(md, ld), 2 * n * np.finfo(float).eps)


def sim_dist(Y, Yref):
    return np.array([tm.rel_dist(y, r) for y, r in zip(Y, Yref)])


# ---- references ------------------------------------------------------------------------------------------------------------------------
def _forcing(name, method, K, m):
    """per kind the forcing columns F_k (m x cols) of X_{k+1} = M X_k + N F_k and the start X_0 selector"""
    u, x0 = signals(name)
    return [tm.inputs_w(us, method) for us in u], x0


def mp_reference(name, method, dt, K, kinds):
    """{kind: Y_ref} by the recurrence in mpmath at DPS digits; all kinds share one pass (their states are columns of one X)"""
    import mpmath as mp
    E, A, B, C = system(name)
    n, m = B.shape
    q = C.shape[0]
    th, beta = tm.theta_beta(method, dt)
    ws, x0 = _forcing(name, method, K, m) if "simulate" in kinds else ([], None)
    with mp.workdps(DPS):
        f = lambda M_: mp.matrix([[mp.mpf(float(v)) for v in row] for row in np.atleast_2d(M_)])
        Em, Am, Bm, Cm = f(E), f(A), f(B), f(C)
        Pinv = mp.inverse(Em - mp.mpf(th) * Am)
        M = 2 * (Pinv * Em) - mp.eye(n) if method == "tustin" else Pinv * Em
        N = mp.mpf(th) * (Pinv * Bm)
        cols, X0 = [], []
        if "step" in kinds:
            cols += [("step", c) for c in range(m)]
            X0 += [[mp.mpf(0)] * n for _ in range(m)]
        if "impulse" in kinds:
            EB = mp.inverse(Em) * Bm
            cols += [("impulse", c) for c in range(m)]
            X0 += [[EB[i, c] for i in range(n)] for c in range(m)]
        if "simulate" in kinds:
            cols += [("simulate", s) for s in range(len(ws))]
            X0 += [[mp.mpf(float(v)) for v in x0[s]] for s in range(len(ws))]
        nc = len(cols)
        X = mp.matrix(n, nc)
        for j in range(nc):
            for i in range(n):
                X[i, j] = X0[j][i]
        out = np.empty((K + 1, q, nc))
        for k in range(K + 1):
            Yk = Cm * X
            for i in range(q):
                for j in range(nc):
                    out[k, i, j] = float(Yk[i, j])
            if k == K:
                break
            F = mp.matrix(m, nc)
            for j, (ki, idx) in enumerate(cols):
                if ki == "step":
                    F[idx, j] = mp.mpf(beta)
                elif ki == "simulate":
                    for c in range(m):
                        F[c, j] = mp.mpf(float(ws[idx][k, c]))
            X = M * X + N * F
    return _split(out, cols, kinds, m)


def _split(out, cols, kinds, m):
    res = {}
    for ki in kinds:
        idx = [j for j, (k_, _) in enumerate(cols) if k_ == ki]
        Y = out[:, :, idx]
        res[ki] = np.ascontiguousarray(Y if ki != "simulate" else Y.transpose(2, 0, 1))
    return res


def refined_reference(name, method, dt, K, kinds, steps=REFINE_STEPS):
    """the same at n = 371: P^-1 [E, B] (and E^-1 B) by an LU solve refined `steps` times with numpy.longdouble residuals, the recurrence in
    numpy.longdouble"""
    import scipy.linalg as sla
    LD = np.longdouble
    E, A, B, C = system(name)
    n, m = B.shape
    th, beta = tm.theta_beta(method, dt)

    def solve(Mx, R):
        lu, Ml, Rl = sla.lu_factor(Mx), Mx.astype(LD), R.astype(LD)
        x = sla.lu_solve(lu, R).astype(LD)
        for _ in range(steps):
            x = x + sla.lu_solve(lu, (Rl - Ml @ x).astype(float)).astype(LD)
        return x
    PEB = solve(E - th * A, np.hstack([E, B]))
    M = 2 * PEB[:, :n] - np.eye(n, dtype=LD) if method == "tustin" else PEB[:, :n]
    N = LD(th) * PEB[:, n:]
    ws, x0 = _forcing(name, method, K, m) if "simulate" in kinds else ([], None)
    cols, X0 = [], []
    if "step" in kinds:
        cols += [("step", c) for c in range(m)]
        X0 += [np.zeros(n, dtype=LD)] * m
    if "impulse" in kinds:
        EB = solve(np.array(E), np.array(B))
        cols += [("impulse", c) for c in range(m)]
        X0 += [EB[:, c] for c in range(m)]
    if "simulate" in kinds:
        cols += [("simulate", s) for s in range(len(ws))]
        X0 += [x0[s].astype(LD) for s in range(len(ws))]
    X = np.array(X0, dtype=LD).T
    Cl = C.astype(LD)
    out = np.empty((K + 1, C.shape[0], len(cols)))
    for k in range(K + 1):
        out[k] = (Cl @ X).astype(float)
        if k == K:
            break
        F = np.zeros((m, len(cols)), dtype=LD)
        for j, (ki, idx) in enumerate(cols):
            if ki == "step":
                F[idx, j] = beta
            elif ki == "simulate":
                F[:, j] = ws[idx][k]
        X = M @ X + N @ F
    return _split(out, cols, kinds, m)


def reference(name, method, dt, K, kinds):
    f = refined_reference if system(name)[0].shape[0] > 70 else mp_reference
    return f(name, method, dt, K, kinds)


def model(name, method, kind, block=None, K=None, dt=None):
    E, A, B, C = system(name)
    dt0, K0 = GRID[name]
    dt, K = dt or dt0, K or K0
    if kind == "step":
        return tm.step_response(E, A, B, C, dt, K, method, block)
    if kind == "impulse":
        return tm.impulse_response(E, A, B, C, dt, K, method, block)
    u, x0 = signals(name)
    return np.array([tm.simulate(E, A, B, C, u[s][:K + 1], dt, x0[s], method, block) for s in range(u.shape[0])])


def lapack(name, method, kind):
    E, A, B, C = system(name)
    dt, K = GRID[name]
    if kind != "simulate":
        return tm.sequential(E, A, B, C, dt, K, method, kind)
    u, x0 = signals(name)
    return np.array([tm.sequential(E, A, B, C, dt, K, method, kind, u[s], x0[s]) for s in range(u.shape[0])])


def dist(kind, Y, Yref):
    return sim_dist(Y, Yref).tolist() if kind == "simulate" else tm.rel_dist(Y, Yref)


def exact_step(E, A, B, C, dt, K):
    """the exact step response on t_k = k dt by the zero-order-hold discretisation (scipy.linalg.expm of the augmented matrix)"""
    import scipy.linalg as sla
    n, m = B.shape
    aug = np.zeros((n + m, n + m))
    aug[:n, :n], aug[:n, n:] = np.linalg.solve(E, A), np.linalg.solve(E, B)
    Z = sla.expm(aug * dt)
    Ad, Bd = Z[:n, :n], Z[:n, n:]
    X, out = np.zeros((n, m)), []
    for _ in range(K + 1):
        out.append(C @ X)
        X = Ad @ X + Bd
    return np.array(out)


def order_errors(step_fn):
    """per method the errors max_i ||y(t_i) - y_exact(t_i)||_F / max_i ||y_exact(t_i)||_F on t_i = 0.1 i for dt = 0.1, 0.05, 0.025;
    step_fn(E, A, B, C, dt, K, method) -> (K+1, q, m)"""
    E, A, B, C = system(ORDER_CASE)
    Yex = dec(recorded()["order"]["Y_exact"])
    out = {}
    for me in METHODS:
        errs = []
        for dt in ORDER_DTS:
            K = int(round(ORDER_T / dt))
            stride = int(round(ORDER_DTS[0] / dt))
            errs.append(tm.rel_dist(step_fn(E, A, B, C, dt, K, me)[::stride], Yex))
        out[me] = errs
    return out


def build_record():
    out = dict(dps=DPS, refine_steps=REFINE_STEPS, grid={k: list(v) for k, v in GRID.items()}, cases={}, steady={}, order={})
    for name in CASES:
        dt, K = GRID[name]
        E = system(name)[0]
        out["cases"][name] = {}
        for me in METHODS:
            kinds = [ki for (m_, ki) in present(name) if m_ == me]
            if not kinds:
                continue
            ref = reference(name, me, dt, K, kinds)
            rec = {}
            for ki in kinds:
                md = dist(ki, model(name, me, ki), ref[ki])
                mdl = {str(L): dist(ki, model(name, me, ki, block=L), ref[ki]) for L in MODEL_BLOCKS}
                ld = dist(ki, lapack(name, me, ki), ref[ki])
                rec[ki] = dict(Y_ref=enc(ref[ki], f"{name}/{me}/{ki}"), model_dist=md, model_dist_L=mdl, lapack_dist=ld)
                print(name, me, ki, "model", md, "L", mdl, "lapack", ld, flush=True)
            out["cases"][name][me] = rec
            M, _ = tm.one_step(*system(name)[:3], dt, me)
            out["cases"][name][me]["rho"] = float(np.abs(np.linalg.eigvals(M)).max())
        out["cases"][name]["reference"] = "lu_refined" if E.shape[0] > 70 else "mpmath"
    for name, (dt, K) in STEADY.items():
        E, A, B, C = system(name)
        M, _ = tm.one_step(E, A, B, dt, "tustin")
        rho = float(np.abs(np.linalg.eigvals(M)).max())
        assert rho ** K < 1e-17, (name, rho ** K)
        ref = mp_reference(name, "tustin", dt, K, ["step"])["step"]
        Ym = tm.step_response(E, A, B, C, dt, K, "tustin")
        out["steady"][name] = dict(dt=dt, K=K, rho_K=rho ** K, Y_last=enc(ref[-1], f"steady/{name}"), model_dist=tm.rel_dist(Ym, ref),
                                   lapack_dist=tm.rel_dist(tm.sequential(E, A, B, C, dt, K, "tustin", "step"), ref),
                                   model_last_dist=float(np.linalg.norm(Ym[-1] - ref[-1]) / np.linalg.norm(ref[-1])))
        print("steady", name, {k: v for k, v in out["steady"][name].items() if k != "Y_last"}, flush=True)
    E, A, B, C = system(ORDER_CASE)
    Yex = exact_step(E, A, B, C, ORDER_DTS[0], int(round(ORDER_T / ORDER_DTS[0])))
    fine = exact_step(E, A, B, C, ORDER_DTS[-1], int(round(ORDER_T / ORDER_DTS[-1])))[::4]
    assert tm.rel_dist(fine, Yex) < 1e-12
    out["order"] = dict(case=ORDER_CASE, T=ORDER_T, dts=list(ORDER_DTS), Y_exact=enc(Yex, "order/Y_exact"))
    return out


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")]
    rec = build_record()
    np.savez_compressed(arrays_path(), **_NEW_ARRAYS)
    arrays.cache_clear()
    with open(record_path(), "w") as fh:
        json.dump(rec, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    recorded.cache_clear()
    errs = order_errors(lambda E, A, B, C, dt, K, me: tm.step_response(E, A, B, C, dt, K, me))
    rec["order"]["model_errors"] = errs
    rec["order"]["model_ratios"] = {me: [e[0] / e[1], e[1] / e[2]] for me, e in errs.items()}
    print("order", rec["order"]["model_ratios"])
    with open(record_path(), "w") as fh:
        json.dump(rec, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("bytes", os.path.getsize(record_path()), os.path.getsize(arrays_path()))
