"""Host NumPy model of the device's tournament-pivoting Gauss-Jordan inversion (csrc/dense_gj.hip: k_gj_tslu, k_gj_swap, k_gj_apply,
k_gj_unpivot, gj_invert_tournament), step for step:

  per panel of nb columns J = k .. k+kb-1
    selection rounds: the candidate rows (rows k .. n-1 at first) in groups of `slab`; each group runs partial-pivot Gauss-Jordan on its
      rows of the panel (ties keep the smaller position, NaN never wins, a pivot-row entry equal to the pivot scales to exactly 1) and
      hands on its kb pivot rows in pivot order; a group without a usable pivot in a column keeps the row in place.  Rounds repeat until
      one group holds every candidate: that final round flags an exactly zero or non-finite pivot as singular, or else yields the
      winners, P^-1 (its top kb rows after elimination) and log|det P|
    interchanges: the winners as an ordered LAPACK-style swap list piv[k .. k+kb), applied to every column
    apply: A(J_rows, J) = P^-1, A(O, J) = -A(O, J) P^-1 on every other row; Pn = A(:, J) - I on the panel rows
    update: A(:, c) += Pn A(J_rows, c) for every column c outside J
  unpivot: the column interchanges in reverse order.
"""
import numpy as np

SLAB = 512     # GJ_THREADS: rows per workgroup of a selection round
NB = 32        # GJ_TSLU_NB


def _round(a, org, kb, final):
    """partial-pivot Gauss-Jordan on one group's rows a (m x kb) with original row indices org.
    Returns (org in pivot order, a after elimination, log|det|), or None (final round, singular)."""
    a = a.copy()
    org = org.copy()
    m = a.shape[0]
    ld = 0.0
    for jj in range(kb):
        j = jj
        best, p = -1.0, m
        if j < m:
            col = np.abs(a[j:, jj])
            ok = ~np.isnan(col)
            if ok.any():
                v = np.where(ok, col, -1.0)
                i = int(np.argmax(v))            # first maximum: ties keep the smaller position
                best, p = float(v[i]), j + i
        bad = not (best > 0.0) or p >= m or not np.isfinite(best)
        if bad:
            if final:
                return None
            continue
        a[[j, p]] = a[[p, j]]
        org[[j, p]] = org[[p, j]]
        pv = a[j, jj]
        dinv = 1.0 / pv
        s = np.where(a[j] == pv, 1.0, a[j] * dinv)
        f = a[:, jj].copy()
        a = a - np.outer(f, s)
        a[:, jj] = -f * dinv
        a[j] = s
        a[j, jj] = dinv
        ld += np.log(abs(pv))
    return org, a, ld


def select(Apanel, k, kb, slab=SLAB):
    """the tournament on the panel columns Apanel (n x kb, the current A(:, J)): (winners, P^-1, log|det P|) or None (singular)"""
    n = Apanel.shape[0]
    assert slab > kb, "a round must shrink the candidate list"
    cand = np.arange(k, n)
    while True:
        G = -(-len(cand) // slab)
        if G == 1:
            r = _round(Apanel[cand], cand, kb, True)
            if r is None:
                return None
            org, a, ld = r
            return org[:kb], a[:kb].copy(), ld
        out = []
        for g in range(G):
            sub = cand[g * slab:(g + 1) * slab]
            org, _, _ = _round(Apanel[sub], sub, kb, False)
            out.append(org[:min(kb, len(sub))])
        cand = np.concatenate(out)


def swap_list(win, k):
    """the winners (original row indices, in pivot order) as the interchanges piv[k + jj] (swap row k + jj with row piv[k + jj] >= k + jj)"""
    occ, loc, piv = {}, {}, []
    for jj, w in enumerate(win):
        d = k + jj
        p = loc.get(int(w), int(w))
        y = occ.get(d, d)
        piv.append(p)
        occ[p] = y; loc[y] = p
        occ[d] = int(w); loc[int(w)] = d
    return np.array(piv, dtype=np.int64)


def tslu_invert(A, nb=NB, slab=SLAB):
    """(inv(A), piv, log|det A|, singular)"""
    A = np.array(A, dtype=float, copy=True)
    n = A.shape[0]
    piv = np.arange(n)
    logdet = 0.0
    for k in range(0, n, nb):
        kb = min(nb, n - k)
        J = slice(k, k + kb)
        r = select(A[:, J], k, kb, slab)
        if r is None:
            return None, None, None, True
        win, Pinv, ld = r
        logdet += ld
        piv[J] = swap_list(win, k)
        for jj in range(kb):
            j, p = k + jj, piv[k + jj]
            if p != j:
                A[[j, p]] = A[[p, j]]
        W = A[J].copy()
        Pn = -A[:, J] @ Pinv
        Pn[J] = Pinv - np.eye(kb)
        A[:, J] = Pn
        A[J, J] += np.eye(kb)
        A[:, :k] += Pn @ W[:, :k]
        A[:, k + kb:] += Pn @ W[:, k + kb:]
    for j in range(n - 1, -1, -1):
        p = piv[j]
        if p != j:
            A[:, [j, p]] = A[:, [p, j]]
    return A, piv, logdet, False


def pivot_forcing(n):
    """kron(I, [[0, 1], [-1, -1]]) (a trailing -1 for odd n): zero leading diagonal entries force an interchange in every other column"""
    blk = np.array([[0.0, 1.0], [-1.0, -1.0]])
    A = np.zeros((n, n))
    A[:n - n % 2, :n - n % 2] = np.kron(np.eye(n // 2), blk)
    if n % 2:
        A[-1, -1] = -1.0
    return A
