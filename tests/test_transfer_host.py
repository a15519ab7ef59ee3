"""CPU side of the complex Gauss-Jordan inversion and of the transfer function at complex points (csrc/dense_cgj.hip, csrc/transfer_eval.hip):
the NumPy model (tests/_cgj_model.py) against LAPACK, the block identity of the update, the record tests/golden/transfer_complex.json, the chunk
arithmetic of the complex path (csrc/freq_chunk.hpp, compiled alone with g++) against brute force, and the argument errors of the Python layer,
which are raised before anything touches a device."""
import os
import subprocess

import numpy as np
import pytest

import dre_amd as D
import _cgj_model as cm
import _freq_cases as fc
import _transfer_cases as tc
from conftest import ROOT

EPS = np.finfo(float).eps
CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")


def test_version_is_at_least_115_and_the_symbols_exist():
    lib = D._lib.load()
    assert lib.dre_version() >= 115
    for name in ("dre_dense_invert_complex_batched", "dre_transfer_eval", "dre_transfer_eval_batched"):
        assert hasattr(lib, name)
    for name in ("dense_invert_complex", "dense_invert_complex_batch", "transfer_function", "transfer_function_batch"):
        assert callable(getattr(D, name))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 31, 33, 70, 513])
def test_model_inversion_against_lapack(n):
    A = cm.test_matrix(n)
    X, piv, ld = cm.invert(A)
    Xl = np.linalg.inv(A)
    cond = np.linalg.cond(A)
    assert np.linalg.norm(X - Xl) <= 10 * n * EPS * cond * np.linalg.norm(Xl)
    assert cm.full_residual(A, X) <= 10 * n * EPS * cond
    ref = np.linalg.slogdet(A)[1]
    assert abs(ld - ref) <= n * EPS * max(abs(ref), 1.0)
    assert np.array_equal(piv, cm.unblocked_pivots(A))
    assert (piv >= np.arange(n)).all()


def test_model_takes_an_interchange_at_every_step_and_flags_singular_columns():
    A = tc.inversion_matrix("rev33")
    X, piv, _ = cm.invert(A)
    assert (piv[:16] == 32 - np.arange(16)).all() and cm.full_residual(A, X) <= 100 * 33 * EPS
    Z = cm.test_matrix(33)
    Z[:, 20] = 0.0
    with pytest.raises(cm.Singular):
        cm.invert(Z)
    Z = cm.test_matrix(33)
    Z[5, 17] = np.nan
    with pytest.raises(cm.Singular):
        cm.invert(Z)


def test_model_reciprocal_is_smiths():
    for p in (3.0 + 4.0j, 4.0 - 3.0j, 2.0 + 0.0j, 0.0 - 2.0j, complex(2.0 ** 600, 2.0 ** 599), complex(2.0 ** -600, -2.0 ** -601)):
        dr, di = cm.reciprocal(p.real, p.imag)
        z = complex(dr, di)
        assert np.isfinite(z) and abs(z * p - 1.0) <= 4 * EPS
    assert cm.reciprocal(2.0, 0.0) == (0.5, 0.0) and cm.reciprocal(0.0, 2.0) == (0.0, -0.5)


def test_block_identity_of_the_update():
    rng = np.random.default_rng(115)
    n, kb = 37, 5
    Cc, P, W = (rng.standard_normal(s) + 1j * rng.standard_normal(s) for s in ((n, n), (n, kb), (kb, n)))
    Cr, Ci = cm.block_update(Cc.real, Cc.imag, P.real, P.imag, W.real, W.imag)
    want = Cc + P @ W
    assert np.linalg.norm(Cr + 1j * Ci - want) <= 8 * kb * EPS * np.linalg.norm(want)
    assert cm.block_form(W.real, W.imag).shape == (2 * kb, 2 * n)


@pytest.mark.parametrize("name", fc.CASES)
def test_complex_model_against_the_frequency_record(name):
    """the model at s = i w stays inside the bound of the existing frequency-response tests, and reproduces its recorded distances"""
    E, A, B, C = fc.system(name)
    om, Href, md, ld = fc.recorded_case(name)
    n = E.shape[0]
    d = cm.rel_dist(cm.transfer(E, A, B, C, 1j * om), Href)
    rec = np.array(tc.recorded()["freq"][name]["model_dist"])
    print(name, "model", d, "recorded", rec, "lapack", ld)
    for k in range(len(om)):
        old_bound = max(10.0 * max(md[k], ld[k]), 2 * n * EPS)
        assert d[k] <= old_bound and rec[k] <= old_bound, (name, om[k])
        assert d[k] <= max(10.0 * max(rec[k], ld[k]), n * EPS)           # the GPU test's bound holds for the model on this machine


def test_the_refinement_step_at_a_decayed_response():
    """pencil371 at w = 1e3, where |H| is 1e-2 of |C| |X| |B| and the embedding's unrefined H is off by 9e-13: the complex panel
    forms the panel's rows of the update as M W, not as W + (M - I) W, and its unrefined H is inside the bound already; the step is kept as
    the device does it and must not take the result out of the bound"""
    E, A, B, C = fc.system("pencil371")
    om, Href, md, ld = fc.recorded_case("pencil371")
    k = int(np.argmax(om))
    bound = max(10.0 * max(md[k], ld[k]), 2 * 371 * EPS)
    d0 = cm.rel_dist(cm.transfer(E, A, B, C, [1j * om[k]], refine=False), Href[k:k + 1])[0]
    d1 = cm.rel_dist(cm.transfer(E, A, B, C, [1j * om[k]]), Href[k:k + 1])[0]
    print(f"w = {om[k]}: unrefined {d0:.2e}, refined {d1:.2e}, bound {bound:.2e}")
    assert d0 <= bound and d1 <= bound


@pytest.mark.parametrize("name", tc.POINT_CASES)
def test_record_of_the_complex_points(name):
    E, A, B, C = fc.system(name)
    s, Href, md, ld = tc.recorded_points(name)
    assert list(s) == list(tc.points(name)) and (s.real > 0).any() and (s.real < 0).any()
    assert Href.shape == (4, C.shape[0], B.shape[1]) and np.isfinite(Href).all()
    d = cm.rel_dist(cm.transfer(E, A, B, C, s), Href)
    dl = cm.rel_dist(cm.lapack(E, A, B, C, s), Href)
    bound = tc.points_bound(name)
    print(name, "model", d, "recorded", md, "lapack", dl, "recorded", ld)
    assert (d <= bound).all() and (dl <= bound).all()


def test_two_points_of_osc12_lie_next_to_a_pole():
    E, A, _, _ = fc.system("osc12")
    poles = np.linalg.eigvals(np.linalg.solve(E, A))
    dist = np.array([np.abs(poles - sk).min() for sk in tc.points("osc12")])
    assert (dist[:2] < 1e-3).all() and (dist[2:] > 1e-2).all()


def test_record_of_the_inversion_cases():
    rec = tc.recorded()["inversion"]
    assert set(rec) == set(tc.INVERSION)
    for key in ("n1_b0", "n33_b1", "n512_b2", "n513_b0", "rev33", "rev513", "n1025_b0"):
        A = tc.inversion_matrix(key)
        r = rec[key]
        assert r["n"] == A.shape[0] and r["kind"] == ("full" if A.shape[0] <= tc.FULL_MAX_N else "probe")
        res = tc.residual(A, cm.invert(A)[0])
        assert res <= max(2.0 * r["model_res"], A.shape[0] * EPS), (key, res, r["model_res"])
        assert abs(r["logabsdet"] - np.linalg.slogdet(A)[1]) <= A.shape[0] * EPS * max(1.0, abs(r["logabsdet"]))


def test_beyond_the_embeddings_limit_the_model_stays_within_a_tenth_of_the_bound():
    """n = 2049, the first order the embedding refuses: the model against LAPACK's complex solve, bound 2 n eps cond_1(i w E - A); the record of
    the GPU test holds this machine's reference to rounding"""
    n = 2049
    E, A, B, C = tc.large_system(n)
    H, cond1 = tc.large_reference(n)
    Hrec, bound_rec = tc.recorded_large(n)
    bound = 2.0 * n * EPS * cond1
    assert np.allclose(bound, bound_rec, rtol=1e-6) and (cm.rel_dist(Hrec, H) <= 0.1 * bound).all()
    d = cm.rel_dist(cm.transfer(E, A, B, C, 1j * tc.LARGE_OMEGA), H)
    print("model", d, "bound", bound)
    assert (d <= 0.1 * bound).all()


# ---- the chunk plan of the complex path, compiled alone with the host compiler -----------------------------------------------------------
PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "freq_chunk.hpp"
int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const dre::FrChunkPlan p = dre::fr_chunk_plan_c(std::strtoull(argv[1], nullptr, 10), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                                    std::atoll(argv[5]), std::atoi(argv[6]));
    std::printf("%d %lld %d %llu %d\n", p.chunk, p.chunks, p.err, dre::fr_member_doubles_c(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])),
                dre::fr_panel_nb_c(std::atoi(argv[2])));
    return 0;
}
"""


def _build_plan(d, flags):
    src = d / "plan_c.cpp"
    src.write_text(PLAN_MAIN)
    exe = d / "plan_c"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(exe)], check=True)

    def run(free, n, m, q, members, forced):
        out = subprocess.run([str(exe)] + [str(v) for v in (free, n, m, q, members, forced)], check=True, capture_output=True, text=True).stdout.split()
        return dict(chunk=int(out[0]), chunks=int(out[1]), err=int(out[2]), per=int(out[3]), nb=int(out[4]))
    return run


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return _build_plan(tmp_path_factory.mktemp("tf_plan"), [])


def _per(n, m, q):
    return 2 * n * n + 6 * n * cm.panel_nb(n) + 6 * n * m + 2 * q * m + n // 2 + 1 + 22


def _brute(free, n, m, q, members, forced):
    per = _per(n, m, q)
    if forced:
        c = min(forced, members)
        return (c, -(-members // c), 0) if c * per <= free else (0, 0, 2)
    c = 0
    for t in range(1, min(members, 65535) + 1):
        if t * per > free:
            break
        c = t
    return (c, -(-members // c), 0) if c else (0, 0, 2)


def test_chunk_plan_against_brute_force(plan):
    rng = np.random.default_rng(115)
    for n, m, q in ((1, 1, 1), (8, 2, 3), (371, 7, 6), (768, 3, 2), (1025, 1, 5), (2049, 4, 4), (4096, 1, 1)):
        per = _per(n, m, q)
        for members in (1, 2, 7, 60, 1000):
            for free in (per - 1, per, 2 * per + 1, 7 * per - 1, 59 * per, 60 * per, int(rng.integers(1, 2000)) * per + int(rng.integers(0, per))):
                for forced in (0, 1, 3, 60):
                    got = plan(free, n, m, q, members, forced)
                    assert got["per"] == per and got["nb"] == cm.panel_nb(n)
                    assert (got["chunk"], got["chunks"], got["err"]) == _brute(free, n, m, q, members, forced), (n, m, q, members, free, forced)


def test_chunk_plan_panel_widths_follow_the_complex_panels_table(plan):
    # cgj_batch_nb: R = ceil(n / 512) rows per thread, 32 columns at R = 1, 16 up to 3, 8 up to 5, 4 above
    for n, want in ((1, 32), (512, 32), (513, 16), (1536, 16), (1537, 8), (2560, 8), (2561, 4), (4096, 4)):
        assert plan(10 ** 12, n, 1, 1, 1, 0)["nb"] == want


def test_chunk_plan_forced_chunk_of_one_and_too_little_memory(plan):
    per = _per(371, 7, 6)
    assert plan(per, 371, 7, 6, 60, 1) == dict(chunk=1, chunks=60, err=0, per=per, nb=32)
    assert plan(per, 371, 7, 6, 60, 0)["chunk"] == 1
    for forced in (0, 1, 60):
        assert plan(per - 1, 371, 7, 6, 60, forced)["err"] == 2          # less than one member: an error, not a chunk of 0
    assert plan(0, 1, 1, 1, 1, 0)["err"] == 2
    assert plan(59 * per, 371, 7, 6, 60, 60)["err"] == 2                 # a forced chunk is not cut to what fits


def test_chunk_plan_at_the_integer_limits(plan):
    imax, lmax, umax = 2 ** 31 - 1, 2 ** 63 - 1, 2 ** 64 - 1
    got = plan(umax, 1, 1, 1, lmax, 0)
    assert (got["chunk"], got["err"]) == (65535, 0) and got["chunks"] == -(-lmax // 65535)
    assert plan(umax, 1, 1, 1, lmax, 1)["chunks"] == lmax
    # the largest shapes: the count is formed in 128 bits
    n, m, q = 2 * 10 ** 9, 1000, imax
    per = _per(n, m, q)
    assert 2 ** 62 < per < 2 ** 63
    got = plan(umax, n, m, q, 5, 0)
    assert got["per"] == per and (got["chunk"], got["chunks"], got["err"]) == (umax // per, -(-5 // (umax // per)), 0)
    assert plan(per - 1, n, m, q, 5, 0)["err"] == 2
    # a member beyond 63 bits is refused, not wrapped
    assert plan(umax, imax, imax, imax, 5, 0) == dict(chunk=0, chunks=0, err=1, per=0, nb=4)
    for args in ((10 ** 9, 0, 1, 1, 1, 0), (10 ** 9, 1, 0, 1, 1, 0), (10 ** 9, 1, 1, 0, 1, 0), (10 ** 9, 1, 1, 1, 0, 0), (10 ** 9, 1, 1, 1, 1, -1),
                 (10 ** 9, 1, 1, 1, 1, 65536), (10 ** 9, -5, 1, 1, 1, 0)):
        assert plan(*args)["err"] == 1, args


def test_chunk_plan_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the stand-alone program over the chunk functions, built with -fsanitize=address,undefined and run once on the CPU"""
    san = _build_plan(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    imax, umax = 2 ** 31 - 1, 2 ** 64 - 1
    assert san(umax, imax, imax, imax, 5, 0)["err"] == 1
    assert san(10 ** 12, 4096, 7, 6, 60, 0)["chunk"] == 60
    assert san(_per(371, 7, 6) - 1, 371, 7, 6, 60, 1)["err"] == 2


# ---- argument errors of the Python layer: raised before a context is asked for ------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("the device was touched")


def test_argument_errors_of_the_transfer_function():
    E, A, B, C = fc.system("one_panel8")
    ctx = _NoDevice()
    bad = [
        dict(s=[]), dict(s=[1.0, complex(np.nan, 0.0)]), dict(s=[complex(0.0, np.inf)]), dict(s=[[1.0, 2.0]]), dict(s=[1.0], errors="ignore"),
        dict(s=[1.0], chunk=0), dict(s=[1.0], chunk=65536), dict(s=[1.0], chunk=1.5), dict(s=[1.0], chunk=True), dict(s=[1.0], D=np.zeros((2, 2))),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="nothing was run on the device"):
            D.transfer_function(E, A, B, C, ctx=ctx, **kw)
    for mats in ((E[:7], A, B, C), (E, A[:, :7], B, C), (E, A, B[:7], C), (E, A, B, C[:, :7]), (E, A, B[:, :0], C), (E, A, B, C[:0])):
        with pytest.raises(ValueError, match="nothing was run on the device"):
            D.transfer_function(*mats, [1.0], ctx=ctx)
    with pytest.raises(TypeError, match="nothing was run on the device"):
        D.transfer_function("E", A, B, C, [1.0], ctx=ctx)
    big = np.zeros((4097, 4097))
    with pytest.raises(ValueError, match="n <= 4096"):
        D.transfer_function(big, big, np.zeros((4097, 1)), np.zeros((1, 4097)), [1.0], ctx=ctx)
    # the ensemble
    with pytest.raises(ValueError, match="empty list"):
        D.transfer_function_batch([], [1.0], ctx=ctx)
    with pytest.raises(TypeError, match="tuple"):
        D.transfer_function_batch([(E, A, B)], [1.0], ctx=ctx)
    with pytest.raises(ValueError, match="share n, m"):
        D.transfer_function_batch([(E, A, B, C), (E, A, B[:, :1], C)], [1.0], ctx=ctx)
    with pytest.raises(ValueError, match="non-finite"):
        D.transfer_function_batch([(E, A, B, C)], [complex(np.nan, 1.0)], ctx=ctx)


def test_argument_errors_of_the_method_switch():
    E, A, B, C = fc.system("one_panel8")
    ctx = _NoDevice()
    rom = D.ReducedModel(np.eye(2), -np.eye(2), np.ones((2, 2)), np.ones((3, 2)), np.array([1.0, 0.5, 0.1]), np.zeros((8, 2)), np.zeros((8, 2)))
    calls = [
        lambda **kw: D.freq_response(E, A, B, C, [1.0], ctx=ctx, **kw),
        lambda **kw: D.freq_response_batch([(E, A, B, C)], [1.0], ctx=ctx, **kw),
        lambda **kw: D.sigma_response(E, A, B, C, [1.0], ctx=ctx, **kw),
        lambda **kw: D.bt_error(E, A, B, C, rom, [1.0], ctx=ctx, **kw),
        lambda **kw: rom.freq_response([1.0], ctx=ctx, **kw),
    ]
    for f in calls:
        for method in ("Complex", "lu", None, 1):
            with pytest.raises(ValueError, match="method must be"):
                f(method=method)
    lq = D.LQGReducedModel(np.eye(2), -np.eye(2), np.ones((2, 2)), np.ones((3, 2)), np.ones(8), np.zeros((8, 2)), np.zeros((8, 2)), np.ones((2, 2)),
                           np.ones((2, 3)), -np.eye(2), np.zeros((2, 8)))
    with pytest.raises(ValueError, match="method must be"):
        D.lqg_error(E, A, B, C, lq, [1.0], ctx=ctx, method="schur")
    with pytest.raises(ValueError, match="method must be"):
        lq.freq_response([1.0], ctx=ctx, method="schur")
    # the limits: n <= 2048 for the embedding only, n <= 4096 for the complex method; a non-finite frequency with either
    big = np.zeros((2049, 2049))
    with pytest.raises(ValueError, match="n <= 2048"):
        D.freq_response(big, big, np.zeros((2049, 1)), np.zeros((1, 2049)), [1.0], ctx=ctx, method="embedding")
    with pytest.raises(AssertionError, match="the device was touched"):          # accepted: the first thing after the checks is the context
        D.freq_response(big, big, np.zeros((2049, 1)), np.zeros((1, 2049)), [1.0], ctx=ctx, method="complex")
    huge = np.zeros((4097, 4097))
    with pytest.raises(ValueError, match="n <= 4096"):
        D.freq_response(huge, huge, np.zeros((4097, 1)), np.zeros((1, 4097)), [1.0], ctx=ctx, method="complex")
    with pytest.raises(ValueError, match="non-finite"):
        D.freq_response(E, A, B, C, [np.nan], ctx=ctx, method="complex")


def test_argument_errors_of_the_complex_inversion():
    ctx = _NoDevice()
    A = cm.test_matrix(5)
    with pytest.raises(ValueError, match="empty list"):
        D.dense_invert_complex_batch([], ctx=ctx)
    with pytest.raises(ValueError, match="nothing was run on the device"):
        D.dense_invert_complex_batch([A, A[:4, :4]], ctx=ctx)
    with pytest.raises(ValueError, match="nothing was run on the device"):
        D.dense_invert_complex_batch([A[:, :4]], ctx=ctx)
    with pytest.raises(ValueError, match="nothing was run on the device"):
        D.dense_invert_complex_batch([A], errors="ignore", ctx=ctx)
    with pytest.raises(ValueError, match="n <= 4096"):
        D.dense_invert_complex_batch([np.zeros((4097, 4097), dtype=complex)], ctx=ctx)
    with pytest.raises(ValueError, match="square"):
        D.dense_invert_complex(A[:, :4], ctx=ctx)
    with pytest.raises(ValueError, match="square"):
        D.dense_invert_complex(np.ones(5), ctx=ctx)
