"""The matrices and points of the complex inversion and transfer-function tests (tests/test_transfer_host.py, tests/test_gpu_transfer.py) and
of the record tests/golden/transfer_complex.json (written by tests/golden/make_fixtures_transfer.py; the tests read only the JSON)."""
import functools
import json
import os

import numpy as np

import _cgj_model as cm

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(float).eps
MARGIN = 10.0
FULL_MAX_N = 600            # up to here an inverse is checked by the full product A X, above by four probe vectors

# ---- inversion -----------------------------------------------------------------------------------------------------------------------------
BATCH3 = (1, 2, 31, 32, 33, 512)                                     # one panel and its edges (R = 1, width 32), batch 3
SINGLE = (513, 1025, 1537, 2049, 2561, 3073, 3585, 4096)             # one order per further R = 2 .. 8, each with a tail panel, batch 1
REVERSED = (33, 513)                                                 # an interchange at every step
INVERSION = tuple(f"n{n}_b{b}" for n in BATCH3 for b in range(3)) + tuple(f"n{n}_b0" for n in SINGLE) + tuple(f"rev{n}" for n in REVERSED)


def inversion_matrix(key):
    if key.startswith("rev"):
        n = int(key[3:])
        rng = np.random.default_rng(9000 + n)
        return np.eye(n)[::-1] + 0.01 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    n, b = key[1:].split("_b")
    return cm.test_matrix(int(n), int(b))


def residual(A, X):
    return cm.full_residual(A, X) if A.shape[0] <= FULL_MAX_N else cm.probe_residual(A, X)


# ---- complex points ------------------------------------------------------------------------------------------------------------------------
POINT_CASES = ("scalar1", "one_panel8", "osc12", "index1_6", "pencil33", "pencil70")


def points(name):
    """four complex points, Re s of both signs"""
    if name == "scalar1":                    # the pole is at -1.5
        return np.array([0.5 + 1.0j, -0.7 + 2.0j, 2.0 - 3.0j, -3.0 + 0.1j])
    if name == "osc12":                      # poles at -5e-6 +- i wn (wn = 0.5, 1, 2, 3.5, 7, 11): the first two points lie within 1e-3 of one
        return np.array([5e-4 + 2.0j, -4e-4 + 3.5003j, 0.1 + 1.0j, -0.1 - 5.0j])
    if name in ("pencil33", "pencil70"):
        return np.array([0.5 + 1.0j, -0.05 + 0.3j, 10.0 - 20.0j, -1e-3 + 100.0j])
    return np.array([0.3 + 1.0j, -0.2 + 0.5j, 1.5 - 2.0j, -1.0 + 10.0j])


# ---- the record ----------------------------------------------------------------------------------------------------------------------------
def record_path():
    return os.path.join(HERE, "golden", "transfer_complex.json")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


def recorded_points(name):
    """(s, H_ref (4, q, m) complex, model_dist, lapack_dist)"""
    r = recorded()["points"][name]
    return (np.array(r["s_re"]) + 1j * np.array(r["s_im"]), np.array(r["H_re"]) + 1j * np.array(r["H_im"]), np.array(r["model_dist"]),
            np.array(r["lapack_dist"]))


def freq_bound(name):
    """per frequency of _freq_cases: max(10 max(complex model's, LAPACK's recorded distance), n eps)"""
    import _freq_cases as fc
    _, _, _, ld = fc.recorded_case(name)
    n = recorded_n(name)
    return np.maximum(MARGIN * np.maximum(np.array(recorded()["freq"][name]["model_dist"]), ld), n * EPS)


def recorded_n(name):
    import _freq_cases as fc
    return fc.recorded()["cases"][name]["n"]


def points_bound(name):
    _, _, md, ld = recorded_points(name)
    return np.maximum(MARGIN * np.maximum(md, ld), recorded_n(name) * EPS)


def inversion_bound(key):
    r = recorded()["inversion"][key]
    return max(MARGIN * max(r["model_res"], r["lapack_res"]), r["n"] * EPS)


# ---- beyond the embedding's limit ------------------------------------------------------------------------------------------------------------
def large_system(n):
    """E = I + 0.2 randn / sqrt(n), A = -2 I + 0.5 randn / sqrt(n), m = q = 1"""
    rng = np.random.default_rng(40000 + n)
    E = np.eye(n) + 0.2 * rng.standard_normal((n, n)) / np.sqrt(n)
    A = -2.0 * np.eye(n) + 0.5 * rng.standard_normal((n, n)) / np.sqrt(n)
    return E, A, rng.standard_normal((n, 1)), rng.standard_normal((1, n))


LARGE_N = (2049, 4096)
LARGE_OMEGA = np.array([0.5, 20.0])


def large_reference(n):
    """(H_ref (2, 1, 1) from LAPACK's complex solve, cond_1(i w E - A) per frequency): what the record holds"""
    E, A, B, C = large_system(n)
    return cm.lapack(E, A, B, C, 1j * LARGE_OMEGA), np.array([float(np.real(np.linalg.cond(1j * w * E - A, 1))) for w in LARGE_OMEGA])


def recorded_large(n):
    """(H_ref, bound = 2 n eps cond_1(i w E - A) per frequency) from the record"""
    r = recorded()["large"][str(n)]
    return np.array(r["H_re"]) + 1j * np.array(r["H_im"]), 2.0 * n * EPS * np.array(r["cond1"])
