"""The systems and frequencies of the frequency-response tests (tests/test_freq_response_host.py, tests/test_gpu_freq_response.py) and the
record tests/golden/freq_response.json.

Cases (E x' = A x + B u, y = C x):
  scalar1        n = 1
  one_panel8     n = 8: the real form has order 16, exactly one panel
  osc12          a lightly damped oscillator, n = 12: A0 = [[0, I], [-K, -c I]], K = Q diag(wn^2) Q', wn = 0.5, 1, 2, 3.5, 7, 11, c = 1e-5,
                 E = I + 0.1 randn, A = E A0, m = 3, q = 2; frequencies next to and on the resonances (cond(i w E - A) from 6e2 to 1.5e8)
  index1_6       an index-1 descriptor system, n = 6: E = diag(I_4, 0), A_22 regular
  pencil33 / 70 / 371   the systems of tests/_balance_cases.py; pencil33_m1 and pencil33_q1 take one column of B / one row of C
The small systems (n <= 12) are kept in the record, so that every machine tests the same numbers; the pencils come from _balance_cases.

The record holds, per case and frequency, H from mpmath at 50 digits (n <= 70) or, at n = 371, from a complex LU solve refined four times with
numpy.longdouble residuals, and next to it the relative distance ||H - H_ref||_F / ||H_ref||_F of the NumPy model (_freq_response_model.py)
and of LAPACK's complex LU solve.  Regenerate with:  python tests/_freq_cases.py   (needs mpmath; the GPU tests read only the JSON)."""
import functools
import json
import os

import numpy as np

import _freq_response_model as fm

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = ("scalar1", "one_panel8", "osc12", "index1_6")
PENCILS = {"pencil33": 33, "pencil70": 70, "pencil371": 371, "pencil33_m1": 33, "pencil33_q1": 33}
CASES = SMALL + tuple(PENCILS)
DPS = 50
REFINE_STEPS = 4


def record_path():
    return os.path.join(HERE, "golden", "freq_response.json")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


def generate_small(name):
    """(E, A, B, C) of a small case from its seed"""
    if name == "scalar1":
        return np.array([[2.0]]), np.array([[-3.0]]), np.array([[1.5]]), np.array([[0.7]])
    if name == "one_panel8":
        rng = np.random.default_rng(808)
        E = np.eye(8) + 0.2 * rng.standard_normal((8, 8)) / np.sqrt(8.0)
        A = -2.0 * np.eye(8) + 0.5 * rng.standard_normal((8, 8))
        return E, A, rng.standard_normal((8, 2)), rng.standard_normal((3, 8))
    if name == "osc12":
        rng = np.random.default_rng(1212)
        wn = np.array([0.5, 1.0, 2.0, 3.5, 7.0, 11.0])
        Q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
        Kst = (Q * wn ** 2) @ Q.T
        A0 = np.block([[np.zeros((6, 6)), np.eye(6)], [-Kst, -1e-5 * np.eye(6)]])
        E = np.eye(12) + 0.1 * rng.standard_normal((12, 12))
        return E, E @ A0, rng.standard_normal((12, 3)), rng.standard_normal((2, 12))
    if name == "index1_6":
        rng = np.random.default_rng(606)
        E = np.diag([1.0, 1.0, 1.0, 1.0, 0.0, 0.0])
        A = 0.5 * rng.standard_normal((6, 6))
        A[:4, :4] -= 1.5 * np.eye(4)
        A[4:, 4:] = np.array([[2.0, 0.5], [-0.3, 1.5]])
        return E, A, rng.standard_normal((6, 2)), rng.standard_normal((2, 6))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def system(name):
    """(E, A, B, C), read-only"""
    if name in SMALL:
        mats = tuple(np.array(recorded()["systems"][name][k], dtype=float) for k in "EABC")
    else:
        import _balance_cases as bc
        E, A, Bm, Cm = bc.system(PENCILS[name])
        if name.endswith("_m1"):
            Bm = Bm[:, :1]
        if name.endswith("_q1"):
            Cm = Cm[:1]
        mats = tuple(np.array(M, dtype=float) for M in (E, A, Bm, Cm))
    for M in mats:
        M.setflags(write=False)
    return mats


def frequencies(name):
    if name == "scalar1":
        return [0.0, 0.1, 1.0, 10.0, 1e3]
    if name == "one_panel8":
        return [0.0, 0.5, 3.0, 100.0]
    if name == "osc12":
        return [0.0, 0.3, 2.0, 2.0001, 11.0]
    if name == "index1_6":
        return [0.0, 1.0, 10.0, 1e4]
    import _balance_cases as bc
    if name == "pencil33":
        return [0.0] + [float(w) for w in bc.OMEGA[::6]]
    if name == "pencil70":
        return [0.0] + [float(w) for w in bc.OMEGA[::12]]
    if name == "pencil371":
        return [float(bc.OMEGA[i]) for i in (0, 12, 24, 36, 48, 59)]
    return [float(bc.OMEGA[i]) for i in (3, 30, 57)]          # pencil33_m1, pencil33_q1


def recorded_case(name):
    """(omega, H_ref (K, q, m) complex, model_dist, lapack_dist) of the record"""
    r = recorded()["cases"][name]
    return (np.array(r["omega"]), np.array(r["H_re"]) + 1j * np.array(r["H_im"]), np.array(r["model_dist"]), np.array(r["lapack_dist"]))


# ---- references ----------------------------------------------------------------------------------------------------------------------
def mp_transfer(E, A, B, C, w, dps=DPS):
    """H(i w) by an LU solve in mpmath at `dps` digits, rounded to double once"""
    import mpmath as mp
    with mp.workdps(dps):
        n, m, q = E.shape[0], B.shape[1], C.shape[0]
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mp.mpc(-mp.mpf(float(A[i, j])), mp.mpf(float(w)) * mp.mpf(float(E[i, j])))
        LU, p = mp.mp.LU_decomp(M)
        H = np.empty((q, m), dtype=complex)
        for c in range(m):
            x = mp.mp.U_solve(LU, mp.mp.L_solve(LU, mp.matrix([mp.mpf(float(v)) for v in B[:, c]]), p))
            for r in range(q):
                h = mp.fsum(mp.mpf(float(C[r, i])) * x[i] for i in range(n))
                H[r, c] = complex(h)
    return H


def refined_transfer(E, A, B, C, w, steps=REFINE_STEPS):
    """H(i w) by a complex LU solve, refined `steps` times with residuals in numpy.longdouble, the product with C in longdouble"""
    import scipy.linalg as sla
    CL = np.clongdouble
    M = 1j * w * E - A
    lu = sla.lu_factor(M)
    Ml = 1j * CL(w) * E.astype(CL) - A.astype(CL)
    Bl = B.astype(CL)
    x = sla.lu_solve(lu, B.astype(complex)).astype(CL)
    for _ in range(steps):
        r = Bl - Ml @ x
        x = x + sla.lu_solve(lu, r.astype(complex)).astype(CL)
    return (C.astype(CL) @ x).astype(complex)


def reference(name, ks=None):
    """H_ref at the frequencies frequencies(name)[k], k in ks (all when None)"""
    E, A, B, C = system(name)
    om = frequencies(name)
    ks = range(len(om)) if ks is None else ks
    f = refined_transfer if PENCILS.get(name) == 371 else mp_transfer
    return np.array([f(E, A, B, C, om[k]) for k in ks])


def build_record():
    out = dict(dps=DPS, refine_steps=REFINE_STEPS, systems={}, cases={})
    for name in SMALL:
        out["systems"][name] = {k: M.tolist() for k, M in zip("EABC", generate_small(name))}
    for name in CASES:
        E, A, B, C = generate_small(name) if name in SMALL else system(name)
        om = frequencies(name)
        f = refined_transfer if PENCILS.get(name) == 371 else mp_transfer
        H = np.array([f(E, A, B, C, w) for w in om])
        md, ld = fm.rel_dist(fm.freq_response(E, A, B, C, om), H), fm.rel_dist(fm.lapack(E, A, B, C, om), H)
        cond = [float(np.linalg.cond(1j * w * E - A)) for w in om]
        out["cases"][name] = dict(n=E.shape[0], m=B.shape[1], q=C.shape[0], reference="lu_refined" if f is refined_transfer else "mpmath", omega=om,
                                  H_re=H.real.tolist(), H_im=H.imag.tolist(), model_dist=md.tolist(), lapack_dist=ld.tolist(), cond=cond)
        print(name, "cond", " ".join(f"{c:.1e}" for c in cond), "model", " ".join(f"{d:.1e}" for d in md), "lapack", " ".join(f"{d:.1e}" for d in ld))
    return out


if __name__ == "__main__":
    import sys
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "oracle")]
    rec = build_record()
    with open(record_path(), "w") as fh:
        json.dump(rec, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
