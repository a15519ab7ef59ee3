"""Batched dense path, the part that needs no device: the ABI level, the exported symbols, the Python entry points and the argument errors
that `solve_batch` / `dense_invert_batch` raise before any device call."""
import numpy as np
import pytest

import dre_amd as D


def _gdre(n=6, m=2, q=3, tspan=(1.0, 0.0), seed=0):
    rng = np.random.default_rng(seed)
    E = np.eye(n)
    A = -np.eye(n) + 0.1 * rng.standard_normal((n, n))
    return D.GDREProblem(E, A, rng.standard_normal((n, m)), rng.standard_normal((q, n)), np.zeros((n, n)), tspan)


def _gale(n=6, seed=0):
    rng = np.random.default_rng(seed)
    return D.GALEProblem(np.eye(n), -np.eye(n) + 0.1 * rng.standard_normal((n, n)), np.eye(n))


def test_abi_level_and_symbols():
    lib = D._lib.load()
    assert lib.dre_version() >= 105
    for name in ("dre_dense_invert_batched", "dre_dense_gale_solve_batched", "dre_dense_gdre_solve_batched"):
        assert hasattr(lib, name), name
        assert name in D._lib.PROTOTYPES


def test_python_entry_points_exist():
    assert callable(D.solve_batch) and callable(D.dense_invert_batch)
    assert "solve_batch" in D.__all__ and "dense_invert_batch" in D.__all__


def test_empty_list_is_a_value_error():
    with pytest.raises(ValueError):
        D.solve_batch([], D.MatrixSign())
    with pytest.raises(ValueError):
        D.solve_batch([], D.Ros1(D.MatrixSign()), dt=-0.1)
    with pytest.raises(ValueError):
        D.dense_invert_batch([])


@pytest.mark.parametrize("other", [dict(n=7), dict(m=3), dict(q=4)])
def test_members_of_different_shape_are_a_value_error(other):
    with pytest.raises(ValueError):
        D.solve_batch([_gdre(), _gdre(**other)], D.Ros1(D.MatrixSign()), dt=-0.1)


def test_gale_members_of_different_order_are_a_value_error():
    with pytest.raises(ValueError):
        D.solve_batch([_gale(6), _gale(7)], D.MatrixSign())
    with pytest.raises(ValueError):
        D.dense_invert_batch([np.eye(4), np.eye(5)])


def test_mixed_problem_types_are_a_type_error():
    with pytest.raises(TypeError):
        D.solve_batch([_gale(), _gdre()], D.MatrixSign())


@pytest.mark.parametrize("alg", [lambda: D.Ros3(D.MatrixSign()), lambda: D.Ros4(D.MatrixSign()), lambda: D.MatrixSign(), lambda: D.Ros1(D.ADI())])
def test_unsupported_gdre_algorithms_are_a_type_error(alg):
    with pytest.raises(TypeError):
        D.solve_batch([_gdre(), _gdre(seed=1)], alg(), dt=-0.1)


def test_unsupported_gale_algorithm_is_a_type_error():
    with pytest.raises(TypeError):
        D.solve_batch([_gale()], D.Ros1(D.MatrixSign()))
    with pytest.raises(TypeError):
        D.solve_batch([_gale()], D.ADI())


def test_observers_are_a_type_error():
    class Obs:
        pass
    with pytest.raises(TypeError):
        D.solve_batch([_gdre()], D.Ros1(D.MatrixSign()), dt=-0.1, observer=Obs())


def test_low_rank_initial_value_is_a_type_error():
    p = _gdre()
    q = D.GDREProblem(p.E, p.A, p.B, p.C, D.lowrank(np.ones((6, 1)), np.eye(1)), p.tspan)
    with pytest.raises(TypeError):
        D.solve_batch([q], D.Ros1(D.MatrixSign()), dt=-0.1)
