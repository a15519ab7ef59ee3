"""Frequency response on the device (freq_response, sigma_response, freq_response_batch, ReducedModel.freq_response, bt_error;
csrc/freq_response.hip) against the record tests/golden/freq_response.json: H from mpmath at 50 digits (n <= 70) or a refined complex LU
(n = 371), with the NumPy model's and LAPACK's recorded distance to it.

Accuracy bound, per frequency:  ||H_dev - H_ref||_F / ||H_ref||_F <= max(10 x max(model's, LAPACK's recorded distance), 2n eps).  The factor 10
is the project's convention for device against model; the distances come from the record, never from the code under test.
Member independence is bit for bit: a frequency's result does not depend on the other frequencies, their order, their number or the chunk."""
import ctypes as C_

import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _freq_cases as fc

pytestmark = pytest.mark.gpu
MARGIN = 10.0
EPS = np.finfo(float).eps


def _dist(H, Href):
    return np.array([np.linalg.norm(h - r) / np.linalg.norm(r) for h, r in zip(H, Href)])


def _bound(name):
    _, _, md, ld = fc.recorded_case(name)
    n = fc.system(name)[0].shape[0]
    return np.maximum(MARGIN * np.maximum(md, ld), 2 * n * EPS)


@pytest.mark.parametrize("name", fc.CASES)
def test_accuracy_against_the_record(ctx, name):
    """scalar1 (n = 1), one_panel8 (2n = 16, one panel), osc12 (cond up to 1.5e8), index1_6 (singular E), the pencils n = 33, 70 at every
    recorded frequency and n = 371 at its six, m = 1 and q = 1 once each"""
    E, A, B, C = fc.system(name)
    om, Href, md, ld = fc.recorded_case(name)
    H, info = D.freq_response(E, A, B, C, om, ctx=ctx, return_info=True)
    assert H.shape == Href.shape and H.dtype == complex
    assert info["members"] == len(om) and info["order"] == 2 * E.shape[0] and info["chunk"] * info["chunks"] >= len(om)
    d, bound = _dist(H, Href), _bound(name)
    print(name, "device", " ".join(f"{v:.1e}" for v in d), "| model", " ".join(f"{v:.1e}" for v in md), "| lapack", " ".join(f"{v:.1e}" for v in ld),
          "| bound", " ".join(f"{v:.1e}" for v in bound), "| chunk", info["chunk"])
    for k in range(len(om)):
        assert d[k] <= bound[k], (name, om[k], d[k], bound[k])


def test_feedthrough_and_sigma(ctx):
    E, A, B, C = fc.system("osc12")
    om, Href, _, _ = fc.recorded_case("osc12")
    Dm = np.arange(6.0).reshape(2, 3)
    H = D.freq_response(E, A, B, C, om, ctx=ctx)
    assert np.array_equal(D.freq_response(E, A, B, C, om, D=Dm, ctx=ctx), H + Dm)
    S = D.sigma_response(E, A, B, C, om, D=Dm, ctx=ctx)
    assert S.shape == (len(om), 2)
    assert np.array_equal(S, np.linalg.svd(H + Dm, compute_uv=False))
    # Weyl: |sigma_1 - sigma_1^ref| <= ||H - H_ref||_2 <= ||H - H_ref||_F
    S0, Sref = D.sigma_response(E, A, B, C, om, ctx=ctx), np.linalg.svd(Href, compute_uv=False)
    assert np.array_equal(S0, np.linalg.svd(H, compute_uv=False))
    assert (np.abs(S0[:, 0] - Sref[:, 0]) <= _bound("osc12") * np.linalg.norm(Href, axis=(1, 2))).all()


# ---- member independence, bit for bit ---------------------------------------------------------------------------------------------------
def test_order_and_company_do_not_change_a_frequency(ctx):
    E, A, B, C = fc.system("pencil70")
    om = np.array(fc.frequencies("pencil70") + [float(w) for w in bc.OMEGA[1::6]] + [0.25])[:17]
    assert len(om) == 17
    H, info = D.freq_response(E, A, B, C, om, ctx=ctx, return_info=True)
    assert info["chunks"] == 1 and info["chunk"] == 17
    assert np.array_equal(D.freq_response(E, A, B, C, om[::-1], ctx=ctx), H[::-1])
    for k in (0, 5, 16):
        assert np.array_equal(D.freq_response(E, A, B, C, om[k:k + 1], ctx=ctx)[0], H[k])


@pytest.mark.parametrize("chunk", [1, 3])
def test_the_chunk_does_not_change_a_frequency(ctx, chunk):
    E, A, B, C = fc.system("osc12")
    om = [0.0, 0.3, 2.0, 2.0001, 11.0, 0.7, 40.0]
    H = D.freq_response(E, A, B, C, om, ctx=ctx)
    Hc, info = D.freq_response(E, A, B, C, om, chunk=chunk, ctx=ctx, return_info=True)
    assert info["chunk"] == chunk and info["chunks"] == -(-7 // chunk)
    assert np.array_equal(Hc, H)


@pytest.mark.parametrize("chunk", [None, 1, 4])
def test_ensemble_members_equal_the_single_calls(ctx, chunk):
    E, A, B, C = fc.system("pencil33")
    rng = np.random.default_rng(3)
    systems = [(E, A, B, C), (E, A * 1.25, B[:, ::-1].copy(), C), (E + 0.01 * rng.standard_normal(E.shape), A, B, 2.0 * C)]
    om = [0.0, 1e-3, 0.5, 30.0, 1e3]
    H, info = D.freq_response_batch(systems, om, chunk=chunk, ctx=ctx, return_info=True)
    assert H.shape == (3, 5, C.shape[0], B.shape[1]) and info["members"] == 15
    if chunk == 4:
        assert info["chunks"] == 4          # chunks 1 and 2 hold frequencies of two systems each
    for s, sys_ in enumerate(systems):
        assert np.array_equal(H[s], D.freq_response(*sys_, om, ctx=ctx)), s


# ---- omega = 0 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["osc12", "pencil33", "index1_6"])
def test_zero_frequency_is_the_static_gain(ctx, name):
    E, A, B, C = fc.system(name)
    om, Href, _, _ = fc.recorded_case(name)
    assert om[0] == 0.0
    H = D.freq_response(E, A, B, C, [0.0], ctx=ctx)[0]
    bound = _bound(name)[0]
    assert np.linalg.norm(H.imag) <= bound * np.linalg.norm(Href[0])
    assert np.linalg.norm(H.real - Href[0].real) <= bound * np.linalg.norm(Href[0])
    G = -C @ np.linalg.solve(A, B)
    assert np.linalg.norm(H.real - G) <= 2 * bound * np.linalg.norm(G)
    print(name, "||Im H(0)|| / ||H(0)|| =", np.linalg.norm(H.imag) / np.linalg.norm(Href[0]))


# ---- failures -----------------------------------------------------------------------------------------------------------------------------
def _singular_at_zero():
    """a zero row and column in A: i w E - A is singular at w = 0 with an exactly zero pivot column, regular at w = 1"""
    E, A, B, C = (np.array(M) for M in fc.system("one_panel8"))
    A[3, :] = 0.0
    A[:, 3] = 0.0
    E = np.eye(8)
    return E, A, B, C


def test_a_frequency_on_a_pole_fails_alone(ctx):
    E, A, B, C = _singular_at_zero()
    with pytest.raises(D.DREError) as e:
        D.freq_response(E, A, B, C, [0.0, 1.0], ctx=ctx)
    assert e.value.code == -4 and "frequency 0" in str(e.value) and "singular" in str(e.value)
    H, errs = D.freq_response(E, A, B, C, [0.0, 1.0], errors="return", ctx=ctx)
    assert isinstance(errs[0], D.DREError) and errs[0].code == -4 and errs[1] is None
    assert np.isnan(H[0].real).all() and np.isnan(H[0].imag).all()
    Href = C @ np.linalg.solve(1j * E - A, B.astype(complex))
    assert np.linalg.norm(H[1] - Href) <= MARGIN * 16 * EPS * np.linalg.cond(1j * E - A) * np.linalg.norm(Href)
    assert np.array_equal(H[1], D.freq_response(E, A, B, C, [1.0], ctx=ctx)[0])
    S, errs = D.sigma_response(E, A, B, C, [0.0, 1.0], errors="return", ctx=ctx)
    assert np.isnan(S[0]).all() and np.array_equal(S[1], np.linalg.svd(H[1], compute_uv=False)) and errs[0].code == -4
    # a NaN in the system: every frequency of that system, and only that system
    An = A.copy()
    An[0, 0] = np.nan
    good = fc.system("one_panel8")
    Hb, eb = D.freq_response_batch([good, (E, An, B, C)], [0.5, 1.0], errors="return", ctx=ctx)
    assert eb[0] == [None, None] and [x.code for x in eb[1]] == [-4, -4] and "system 1" in str(eb[1][1])
    assert np.isnan(Hb[1]).all() and np.array_equal(Hb[0], D.freq_response(*good, [0.5, 1.0], ctx=ctx))
    # the context lives on
    assert np.isfinite(D.freq_response(*good, [0.0], ctx=ctx)).all()


def test_the_c_entry_rejects_bad_arguments_before_any_launch(ctx):
    E, A, B, C = (ctx.upload(np.asfortranarray(M)) for M in fc.system("one_panel8"))
    lib = ctx.lib
    pd, pi32 = C_.POINTER(C_.c_double), C_.POINTER(C_.c_int32)
    re, im, st = np.full(6 * 4, 7.0), np.full(6 * 4, 7.0), np.full(4, 9, dtype=np.int32)

    def call(Eh, Ah, Bh, Ch, om, K=None, chunk=0):
        w = np.array(om, dtype=float)
        return lib.dre_freq_response(ctx.ptr, Eh.ptr, Ah.ptr, Bh.ptr, Ch.ptr, len(om) if K is None else K, w.ctypes.data_as(pd), chunk,
                                     re.ctypes.data_as(pd), im.ctypes.data_as(pd), st.ctypes.data_as(pi32), None)
    assert call(E, A, B, C, [1.0, np.nan]) == -1 and b"not finite" in lib.dre_last_error(ctx.ptr)
    assert call(E, A, B, C, [np.inf]) == -1
    assert call(E, A, B, C, [1.0], K=0) == -1 and b"K >= 1" in lib.dre_last_error(ctx.ptr)
    assert call(E, A, B, C, [1.0], chunk=-1) == -1 and call(E, A, B, C, [1.0], chunk=65536) == -1
    assert call(E, A, C, C, [1.0]) == -1 and call(E, A, B, B, [1.0]) == -1 and call(B, A, B, C, [1.0]) == -1 and call(E, C, B, C, [1.0]) == -1
    big = ctx.upload(np.zeros((2049, 2049), order="F"))
    assert call(big, big, ctx.upload(np.zeros((2049, 1))), ctx.upload(np.zeros((1, 2049))), [1.0]) == -1 and b"2n <= 4096" in lib.dre_last_error(ctx.ptr)
    arr = (C_.c_void_p * 1)(E.ptr)
    w = np.array([1.0])
    assert lib.dre_freq_response_batched(ctx.ptr, 0, arr, arr, arr, arr, 1, w.ctypes.data_as(pd), 0, re.ctypes.data_as(pd), im.ctypes.data_as(pd),
                                         st.ctypes.data_as(pi32), None) == -1
    # nothing was written
    assert (re == 7.0).all() and (im == 7.0).all() and (st == 9).all()
    # and the call works afterwards, with info
    info = (C_.c_int64 * 2)()
    w = np.array([0.5, 3.0])
    assert lib.dre_freq_response(ctx.ptr, E.ptr, A.ptr, B.ptr, C.ptr, 2, w.ctypes.data_as(pd), 0, re.ctypes.data_as(pd), im.ctypes.data_as(pd),
                                 st.ctypes.data_as(pi32), info) == 0
    assert list(info) == [2, 1] and (st[:2] == 0).all()
    om, Href, _, _ = fc.recorded_case("one_panel8")
    H = (re[:12] + 1j * im[:12]).reshape(2, 2, 3).transpose(0, 2, 1)
    assert (_dist(H, Href[1:3]) <= _bound("one_panel8")[1:3]).all()


# ---- the guarantee, end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r", [(33, 8), (70, 12)])
def test_balanced_truncation_meets_its_bound(ctx, n, r):
    """max_w ||H(iw) - H_r(iw)||_2 <= 2 sum_{i > r} sigma_i on the 60 frequencies of _balance_cases.OMEGA, both responses from the device; the
    maximum within 1 % of what the NumPy helper gives for the same reduced model (the reference alone has bound / error >= 1.99 here)"""
    E, A, Bm, Cm = bc.system(n)
    rom = D.balanced_truncation(E, A, Bm, Cm, order=r, ctx=ctx)
    res = D.bt_error(E, A, Bm, Cm, rom, bc.OMEGA, ctx=ctx)
    Hr = bc.reduced_transfer(dict(order=r, Ar=rom.Ar, Br=rom.Br, Cr=rom.Cr))
    err = np.array([np.linalg.norm(h, 2) for h in bc.golden()[f"H_{n}"] - Hr])
    print(f"n={n} r={r}: device max error {res['max_error']:.6e} at {res['omega_at_max']:.3e}, NumPy {err.max():.6e} at {bc.OMEGA[err.argmax()]:.3e}, "
          f"bound {res['bound']:.6e}, ratio {res['ratio']:.4f}")
    assert res["bound"] == 2.0 * float(np.sum(rom.hsv[r:][::-1]))
    assert res["max_error"] <= res["bound"]
    assert abs(res["max_error"] - err.max()) <= 0.01 * err.max()
    assert res["ratio"] == res["bound"] / res["max_error"] and res["omega_at_max"] in bc.OMEGA
    assert np.array_equal(rom.freq_response(bc.OMEGA[:3], ctx=ctx), D.freq_response(np.eye(r), rom.Ar, rom.Br, rom.Cr, bc.OMEGA[:3], ctx=ctx))
