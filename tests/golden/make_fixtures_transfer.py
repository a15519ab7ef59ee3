"""Writes tests/golden/transfer_complex.json, the record of the complex Gauss-Jordan inversion and of the transfer function at complex points
(tests/test_transfer_host.py, tests/test_gpu_transfer.py).  Figures only, all from the CPU:

  freq        per case of _freq_cases.CASES and frequency: the distance of the complex model (tests/_cgj_model.py: transfer at s = i w) from the
              references that tests/golden/freq_response.json already holds
  points      per case of POINT_CASES four complex points s (Re s of both signs; two of osc12's within 1e-3 of a pole): H(s) from mpmath at 50
              digits, the model's and LAPACK's relative distance from it, cond(s E - A)
  inversion   per matrix of the inversion tests (_transfer_cases.INVERSION): the residual of the model's inverse and of numpy.linalg.inv's,
              ||A X - I||_F / sqrt(n) up to n = 600 and max_v ||A (X v) - v|| / ||v|| over four seeded probe vectors above, and log|det| from
              numpy.linalg.slogdet
  large       the systems beyond the embedding's limit (_transfer_cases.large_system, n = 2049 and 4096) at LARGE_OMEGA: H from LAPACK's complex
              solve and cond_1(i w E - A) from numpy.linalg.cond(., 1)

Run from the repository root:  python tests/golden/make_fixtures_transfer.py [section ...]   (no section: all four; a named section replaces
that section of the existing file.  Needs mpmath for `points`; minutes: the model inverts n = 4096 in NumPy)."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import _cgj_model as cm            # noqa: E402
import _freq_cases as fc           # noqa: E402
import _transfer_cases as tc       # noqa: E402


def mp_transfer(E, A, B, C, s, dps=50):
    """H(s) by an LU solve in mpmath at `dps` digits, rounded to double once"""
    import mpmath as mp
    with mp.workdps(dps):
        n, m, q = E.shape[0], B.shape[1], C.shape[0]
        sm = mp.mpc(mp.mpf(float(s.real)), mp.mpf(float(s.imag)))
        M = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = sm * mp.mpf(float(E[i, j])) - mp.mpf(float(A[i, j]))
        LU, p = mp.mp.LU_decomp(M)
        H = np.empty((q, m), dtype=complex)
        for c in range(m):
            x = mp.mp.U_solve(LU, mp.mp.L_solve(LU, mp.matrix([mp.mpf(float(v)) for v in B[:, c]]), p))
            for r in range(q):
                H[r, c] = complex(mp.fsum(mp.mpf(float(C[r, i])) * x[i] for i in range(n)))
    return H


def build_freq(out):
    out["freq"] = {}
    for name in fc.CASES:
        E, A, B, C = fc.system(name)
        om, Href, _, _ = fc.recorded_case(name)
        d = cm.rel_dist(cm.transfer(E, A, B, C, 1j * om), Href)
        out["freq"][name] = dict(model_dist=d.tolist())
        print("freq", name, " ".join(f"{v:.1e}" for v in d), flush=True)


def build_points(out):
    out["points"] = {}
    for name in tc.POINT_CASES:
        E, A, B, C = fc.system(name)
        s = tc.points(name)
        H = np.array([mp_transfer(E, A, B, C, sk) for sk in s])
        md, ld = cm.rel_dist(cm.transfer(E, A, B, C, s), H), cm.rel_dist(cm.lapack(E, A, B, C, s), H)
        cond = [float(np.linalg.cond(sk * E - A)) for sk in s]
        out["points"][name] = dict(s_re=s.real.tolist(), s_im=s.imag.tolist(), H_re=H.real.tolist(), H_im=H.imag.tolist(), model_dist=md.tolist(),
                                   lapack_dist=ld.tolist(), cond=cond)
        print("points", name, "cond", " ".join(f"{c:.1e}" for c in cond), "model", " ".join(f"{v:.1e}" for v in md), "lapack",
              " ".join(f"{v:.1e}" for v in ld), flush=True)


def build_inversion(out):
    out["inversion"] = {}
    for key in tc.INVERSION:
        A = tc.inversion_matrix(key)
        n = A.shape[0]
        t = time.time()
        res = tc.residual(A, cm.invert(A)[0])
        lap = tc.residual(A, np.linalg.inv(A))
        out["inversion"][key] = dict(n=n, kind="full" if n <= tc.FULL_MAX_N else "probe", model_res=res, lapack_res=lap,
                                     logabsdet=float(np.linalg.slogdet(A)[1]))
        print("inversion", key, f"model {res:.2e} lapack {lap:.2e}  ({time.time() - t:.1f} s)", flush=True)


def build_large(out):
    out["large"] = {}
    for n in tc.LARGE_N:
        H, cond1 = tc.large_reference(n)
        out["large"][str(n)] = dict(omega=tc.LARGE_OMEGA.tolist(), H_re=H.real.tolist(), H_im=H.imag.tolist(), cond1=cond1.tolist())
        print("large", n, "cond_1", " ".join(f"{c:.2e}" for c in cond1), flush=True)


SECTIONS = dict(freq=build_freq, points=build_points, inversion=build_inversion, large=build_large)

if __name__ == "__main__":
    path = os.path.join(HERE, "transfer_complex.json")
    names = sys.argv[1:] or list(SECTIONS)
    rec = dict(dps=50)
    if sys.argv[1:]:
        with open(path) as fh:
            rec = json.load(fh)
    for nm in names:
        SECTIONS[nm](rec)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
