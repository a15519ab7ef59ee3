"""The host model of the tournament-pivoting Gauss-Jordan inversion (tests/_tslu_model.py) against numpy.linalg.inv / slogdet: random,
pivot-forcing and graded matrices, n not a multiple of the panel width, one selection round and several (small slabs stand in for the
device's 512-row workgroups), and exactly singular panels."""
import numpy as np
import pytest
import scipy.linalg as sla

import _tslu_model as tm

EPS = np.finfo(float).eps


def _check(A, nb, slab, tol_fac=100.0):
    X, piv, ld, sing = tm.tslu_invert(A, nb=nb, slab=slab)
    assert not sing
    n = A.shape[0]
    r = np.linalg.norm(A @ X - np.eye(n)) / (np.linalg.norm(A) * np.linalg.norm(X))
    assert r <= tol_fac * n * EPS, r
    s, ldn = np.linalg.slogdet(A)
    assert s != 0 and abs(ld - ldn) <= 1e-12 * max(1.0, abs(ldn))
    assert np.allclose(X, np.linalg.inv(A), rtol=0, atol=1e-9 * np.abs(X).max())
    assert all(piv[j] >= j for j in range(n))
    return X, piv


@pytest.mark.parametrize("n,nb,slab", [(64, 32, 512), (100, 32, 512), (100, 8, 16), (131, 32, 40), (257, 16, 24), (97, 32, 33)])
def test_random(n, nb, slab):
    A = np.random.default_rng(n + nb + slab).standard_normal((n, n))
    _check(A, nb, slab)


@pytest.mark.parametrize("n,slab", [(90, 512), (91, 40), (200, 48)])
def test_pivot_forcing(n, slab):
    A = tm.pivot_forcing(n)
    X, piv = _check(A, 32, slab)
    assert np.array_equal(X, np.linalg.inv(A))           # entries 0, +-1: exact
    odd = np.arange(0, n - n % 2, 2)
    assert np.array_equal(piv[odd], odd + 1)              # every zero diagonal entry swapped with the row below


@pytest.mark.parametrize("slab", [512, 40])
def test_graded(slab):
    n = 150
    rng = np.random.default_rng(5)
    d = np.logspace(0, -8, n)
    A = np.diag(d) @ rng.standard_normal((n, n)) @ np.diag(d[::-1])
    _check(A, 32, slab, tol_fac=1000.0)


def test_one_round_is_partial_pivoting():
    """with every candidate in one group the tournament is partial pivoting: the interchanges are LAPACK's getrf ipiv"""
    n = 120
    A = np.random.default_rng(11).standard_normal((n, n))
    _, piv = _check(A, 32, 512)
    _, ipiv = sla.lu_factor(A)
    assert np.array_equal(piv, ipiv)


def test_swap_list_reproduces_the_winners():
    rng = np.random.default_rng(3)
    n, k = 50, 10
    win = rng.permutation(np.arange(k, n))[:8]
    piv = tm.swap_list(win, k)
    rows = np.arange(n)
    for jj, p in enumerate(piv):
        rows[[k + jj, p]] = rows[[p, k + jj]]
    assert np.array_equal(rows[k:k + 8], win)


@pytest.mark.parametrize("slab", [512, 40])
def test_exactly_singular_is_flagged(slab):
    n = 100
    A = np.random.default_rng(2).standard_normal((n, n))
    Az = A.copy(); Az[:, 40] = 0.0                            # a zero column in a later panel
    assert tm.tslu_invert(Az, slab=slab)[3]
    Ae = A.copy(); Ae[:, 3] = Ae[:, 2]                        # two equal columns of one panel
    assert tm.tslu_invert(Ae, slab=slab)[3]
    Ar = A.copy(); Ar[7] = 0.0                                # a zero row
    assert tm.tslu_invert(Ar, slab=slab)[3]
    An = A.copy(); An[5, 5] = np.nan                          # NaN never passes as a pivot
    X, _, _, sing = tm.tslu_invert(An, slab=slab)
    assert sing or not np.isfinite(X).all()
