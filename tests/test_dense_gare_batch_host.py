"""Batched dense GARE, the part that needs no device: the ABI level, the exported symbol, and the argument errors that `solve_batch`
raises for a list of GAREProblem before any device call."""
import numpy as np
import pytest

import dre_amd as D
from dre_amd.api import _check_batch


def _gare(n=6, m=2, q=3, seed=0):
    rng = np.random.default_rng(seed)
    A = -np.eye(n) + 0.1 * rng.standard_normal((n, n))
    return D.GAREProblem(np.eye(n), A, D.lowrank(rng.standard_normal((n, m)), np.eye(m)), D.lowrank(rng.standard_normal((n, q)), np.eye(q)))


def _gale(n=6):
    return D.GALEProblem(np.eye(n), -np.eye(n), np.eye(n))


def test_abi_level_and_symbol():
    lib = D._lib.load()
    assert lib.dre_version() >= 106
    assert hasattr(lib, "dre_dense_gare_solve_batched")
    assert "dre_dense_gare_solve_batched" in D._lib.PROTOTYPES
    assert len(D._lib.PROTOTYPES["dre_dense_gare_solve_batched"][1]) == 15


def test_a_gare_list_passes_the_checks():
    assert _check_batch([_gare(seed=0), _gare(seed=1), _gare(seed=2)], D.MatrixSign(), None) == ("gare", 0)
    assert _check_batch([_gare()], D.MatrixSign(maxiters=25, tol=1e-3), None) == ("gare", 0)


@pytest.mark.parametrize("other", [dict(n=7), dict(m=3), dict(q=4)])
def test_members_of_different_shape_are_a_value_error(other):
    with pytest.raises(ValueError):
        _check_batch([_gare(), _gare(**other)], D.MatrixSign(), None)
    with pytest.raises(ValueError):
        D.solve_batch([_gare(), _gare(**other)], D.MatrixSign())


def test_dt_and_save_state_are_a_value_error():
    with pytest.raises(ValueError):
        D.solve_batch([_gare(), _gare(seed=1)], D.MatrixSign(), dt=-0.1)
    with pytest.raises(ValueError):
        D.solve_batch([_gare(), _gare(seed=1)], D.MatrixSign(), save_state=True)


def test_an_observer_is_a_type_error():
    with pytest.raises(TypeError):
        D.solve_batch([_gare()], D.MatrixSign(), observer=object())


@pytest.mark.parametrize("alg", [D.Ros1(D.MatrixSign()), D.Ros2(D.MatrixSign()), D.Newton(), D.ADI()])
def test_another_algorithm_is_a_type_error(alg):
    with pytest.raises(TypeError):
        _check_batch([_gare(), _gare(seed=1)], alg, None)
    with pytest.raises(TypeError):
        D.solve_batch([_gare(), _gare(seed=1)], alg)


def test_mixed_gare_and_gale_is_a_type_error():
    with pytest.raises(TypeError):
        _check_batch([_gare(), _gale()], D.MatrixSign(), None)
    with pytest.raises(TypeError):
        D.solve_batch([_gale(), _gare()], D.MatrixSign())
