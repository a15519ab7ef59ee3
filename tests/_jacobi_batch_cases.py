"""The members of the batched block Jacobi tests (tests/test_gpu_jacobi_batch.py) and the systems of the ensemble balanced-truncation tests
(tests/test_gpu_balance_batch.py, tests/test_jacobi_batch_host.py) with their CPU references, computed once per process.

SVD and eigensolver members: per shape a batch of four: two random members, one that is finished after the first sweep (the zero matrix for the
SVD, a diagonal matrix for the eigensolver) and one graded member that needs more sweeps than the random ones.

Balanced truncation: the systems of tests/_balance_cases.py at n = 33 and 70 and two variants each, (E, A - s E, B, C) with s = 0.05 and 0.2 (the
pencil's eigenvalues move left by s, so the variants stay c-stable).
reference(n, i)   tests/_balance_cases.py's own reference chain on member i: oracle.lyap_dense Gramians, eigh factors with the n eps rule,
                  numpy.linalg.svd, the products in extended precision.  Recorded in tests/golden/balance_batch_reference.npz.
chain(n, i)       the NumPy restatement of the batched route: the dense sign model's Gramians (tests/_sign_model.py, what
                  dre_dense_gale_solve_batched iterates), eigh factors with eigenvalues at or below n eps lambda_max set to zero, every
                  Z_o'E Z_c zero padded to the batch's common shape, the SVD model of tests/_svd_jacobi_model.py on the padded matrix, then the
                  steps of csrc/balance.hip.  Its distances from the reference are recorded in tests/golden/balance_batch_model.json.
Regenerate both records with:  python tests/_jacobi_batch_cases.py   (tests/ and oracle/ on the path)
"""
import functools
import json
import os

import numpy as np

import _svd_jacobi_model as sv

EPS = np.finfo(float).eps
SVD_SHAPES = ((40, 33), (70, 17), (33, 32), (300, 32), (33, 40), (23, 1))
EIG_ORDERS = (1, 32, 33, 70)


# ---- SVD and eigensolver members ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def svd_members(m, w):
    """[random, random, zero, graded] of shape m x w"""
    rng = np.random.default_rng(7000 + 100 * m + w)
    k = min(m, w)
    graded = sv._graded(max(m, w), k, -12.0, 7100 + m + w)
    graded = graded if m >= w else graded.T
    out = [rng.standard_normal((m, w)), rng.standard_normal((m, w)), np.zeros((m, w)), np.ascontiguousarray(graded)]
    for A in out:
        A.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def eig_members(q):
    """[random, random, diagonal, graded] symmetric matrices of order q"""
    rng = np.random.default_rng(7500 + q)
    out = []
    for _ in range(2):
        A = rng.standard_normal((q, q))
        out.append(0.5 * (A + A.T))
    out.append(np.diag(np.linspace(1.0, 2.0, q)))
    Qm = np.linalg.qr(rng.standard_normal((q, q)))[0]
    A = (Qm * np.logspace(0.0, -12.0, q)) @ Qm.T
    out.append(0.5 * (A + A.T))
    for A in out:
        A.setflags(write=False)
    return out


# ---- the ensembles of the balanced-truncation tests ------------------------------------------------------------------------------------------
SIZES = (33, 70)
SHIFTS = (0.0, 0.05, 0.2)
ORDER = 8


@functools.lru_cache(maxsize=None)
def systems(n):
    """[(E, A - s E, B, C) for s in SHIFTS]"""
    import _balance_cases as bc
    E, A, Bm, Cm = bc.system(n)
    out = []
    for s in SHIFTS:
        As = A - s * E
        As.setflags(write=False)
        out.append((E, As, Bm, Cm))
    return out


@functools.lru_cache(maxsize=None)
def ref_gramians(n, i):
    import dre_oracle as o
    import _balance_cases as bc
    E, A, Bm, Cm = systems(n)[i]
    P, Q = o.lyap_dense(A.T, E.T, Bm @ Bm.T), o.lyap_dense(A, E, Cm.T @ Cm)
    return bc._eigh_factor(P, bc.rank_rtol(n)) + bc._eigh_factor(Q, bc.rank_rtol(n))


@functools.lru_cache(maxsize=None)
def reference(n, i, order=0, tol=1e-8):
    import _balance_cases as bc
    return bc._reference_balance(*systems(n)[i], *ref_gramians(n, i), order, tol)


def zeroed_eigh(X, n):
    """(V, lam) of eigh with the eigenvalues at or below n eps lambda_max set to zero (the rule of balanced_truncation_batch)"""
    lam, V = np.linalg.eigh(X)
    lam = lam.copy()
    lam[lam <= n * EPS * lam.max()] = 0.0
    return V, lam


@functools.lru_cache(maxsize=None)
def model_gramians(n, i):
    """(Lc, dc, Lo, do) as the batched route forms them: member b (E, A, C'C), member B + b (E', A', B B') of one batched sign solve"""
    import _sign_model as sm
    E, A, Bm, Cm = systems(n)[i]
    Q = sm.sign_lyap(A, E, Cm.T @ Cm)[0]
    P = sm.sign_lyap(A.T, E.T, Bm @ Bm.T)[0]
    return zeroed_eigh(P, n) + zeroed_eigh(Q, n)


def padded_svd(shape):
    """the SVD model on M zero padded to `shape`, cut back to M's own blocks: what a member of the batched SVD sees"""
    def fn(M):
        ro, rc = M.shape
        k = min(ro, rc)
        Mp = np.zeros(shape)
        Mp[:ro, :rc] = M
        U, s, V, st = sv.svd(Mp)
        return U[:ro, :], s[:k], V[:rc, :], dict(st, rank=min(st["rank"], k))
    return fn


@functools.lru_cache(maxsize=None)
def padded_shape(n):
    """(max r_o, max r_c) over the batch of the three systems of order n"""
    ranks = [(int((model_gramians(n, i)[3] > 0).sum()), int((model_gramians(n, i)[1] > 0).sum())) for i in range(len(SHIFTS))]
    return max(r[0] for r in ranks), max(r[1] for r in ranks)


@functools.lru_cache(maxsize=None)
def chain(n, i, order=0, tol=1e-8, shape=None):
    return sv.balance(*systems(n)[i], *model_gramians(n, i), order=order, tol=tol, svd_fn=padded_svd(shape or padded_shape(n)))


def h0_norm(n, i):
    E, A, Bm, Cm = systems(n)[i]
    return float(np.linalg.norm(Cm @ np.linalg.solve(-A, Bm), 2))


def errors_against(ref_hsv, Hr_ref, h0, hsv, eye, red):
    """(max |sigma - sigma_ref| / sigma_1, ||W'ET - I||_F, max_w ||H_r - H_r^ref||_2 / ||H(0)||_2) of a reduced model dict(order, Ar, Br, Cr)"""
    import _balance_cases as bc
    k = min(len(ref_hsv), len(hsv))
    return (float(np.abs(hsv[:k] - ref_hsv[:k]).max() / ref_hsv[0]), float(eye), bc.max_norm2(bc.reduced_transfer(red) - Hr_ref) / h0)


@functools.lru_cache(maxsize=None)
def batch_tol(n):
    """(tol, orders): ONE tolerance for the batch of order n (the batched call takes one) at which the reference's order rule is decided by
    more than 10 % on both sides for every member, with the order it gives each member.  Candidates are the geometric means of the two values
    of 2 sum tail / sigma_1 around the orders 6 .. 14 of every member (tests/_balance_cases.py: clear_tol); the one with the widest margin wins."""
    import _balance_cases as bc
    hsv = [reference(n, i, ORDER)["hsv"] for i in range(len(SHIFTS))]
    best = None
    for s in hsv:
        for r in range(6, 15):
            tol = bc.clear_tol(s, r)
            orders = [sv.choose_order(h, len(h), tol) for h in hsv]
            margin = min(min(1.0 - bc.tail_ratio(h, o, tol), bc.tail_ratio(h, o - 1, tol) - 1.0) for h, o in zip(hsv, orders))
            if margin > 0.1 and (best is None or margin > best[0]):
                best = (margin, tol, orders)
    assert best is not None
    return best[1], best[2]


def labels(n, i):
    return (("order8", ORDER), ("tol", batch_tol(n)[1][i]))


def golden_arrays():
    """what the device tests need of reference(n, i): the Hankel singular values, H, ||H(0)||, H_r at order 8 and at the order chosen by tol"""
    import _balance_cases as bc
    out = {}
    for n in SIZES:
        for i in range(len(SHIFTS)):
            ref = reference(n, i, ORDER)
            out[f"hsv_{n}_{i}"] = ref["hsv"]
            out[f"H_{n}_{i}"] = bc.transfer(*systems(n)[i])
            out[f"h0_{n}_{i}"] = np.array(h0_norm(n, i))
            for lab, r in labels(n, i):
                out[f"Hr_{lab}_{n}_{i}"] = bc.reduced_transfer(reference(n, i, r))
    return out


def record():
    """the chain's figures: per member the ranks, the padded shape, the tolerance with its order, and the chain's three distances from the
    reference at order 8 and at the order chosen by the tolerance"""
    import _balance_cases as bc
    out = {}
    for n in SIZES:
        for i in range(len(SHIFTS)):
            ref = reference(n, i, ORDER)
            tol, tol_order = batch_tol(n)[0], batch_tol(n)[1][i]
            for r in (tol_order, tol_order - 1):
                assert not 0.9 <= bc.tail_ratio(ref["hsv"], r, tol) <= 1.1
            assert reference(n, i, 0, tol)["order"] == chain(n, i, 0, tol)["order"] == tol_order
            ch0 = chain(n, i, ORDER)
            rec = dict(ref_r_o=ref["r_o"], ref_r_c=ref["r_c"], r_o=ch0["r_o"], r_c=ch0["r_c"], rank=ch0["rank"], sweeps=ch0["sweeps"],
                       padded_shape=list(padded_shape(n)), tol=tol, tol_order=tol_order)
            for lab, r in labels(n, i):
                ch, rf = chain(n, i, r), reference(n, i, r)
                e = errors_against(rf["hsv"], bc.reduced_transfer(rf), h0_norm(n, i), ch["hsv"], ch["eye_err"], ch)
                rec.update({f"{k}_{lab}": v for k, v in zip(("sigma", "eye", "transfer"), e)})
            out[f"{n}_{i}"] = rec
    return out


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "balance_batch_reference.npz")


def record_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "balance_batch_model.json")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(golden_path()) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    np.savez(golden_path(), **golden_arrays())
    rec = record()
    for k, v in rec.items():
        print(k, v)
    with open(record_path(), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
