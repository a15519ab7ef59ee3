"""The complex Gauss-Jordan inversion (dense_invert_complex[_batch]; csrc/dense_cgj.hip) and the transfer function at complex points
(transfer_function[_batch], method="complex" of the frequency-response family; csrc/transfer_eval.hip) on the device, against the records
tests/golden/transfer_complex.json and tests/golden/freq_response.json.

Accuracy bound, per frequency, point or matrix:  ||._dev - ._ref|| / ||._ref|| <= max(10 x max(recorded complex-model figure, recorded LAPACK
figure), n eps).  The figures come from the record (tests/golden/make_fixtures_transfer.py, CPU only), never from the code under test.  For an
inverse the figure is the residual ||A X - I||_F / sqrt(n) up to n = 600 and max_v ||A (X v) - v|| / ||v|| on four seeded probes above.
Member independence is bit for bit."""
import ctypes as C_

import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _cgj_model as cm
import _freq_cases as fc
import _transfer_cases as tc

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _dist(H, Href):
    return np.array([np.linalg.norm(h - r) / np.linalg.norm(r) for h, r in zip(H, Href)])


def _check_inverse(key, A, out, logdet_abs=False):
    """logdet_abs: |log det| is near zero (|det| about 1), where a tolerance relative to it means nothing: each of the n terms log|pivot| carries
    the relative error of |pivot| (an ulp or two) as an absolute error, so n eps absolute"""
    X, piv, ld = out
    n = A.shape[0]
    rec = tc.recorded()["inversion"][key]
    res, bound = tc.residual(A, X), tc.inversion_bound(key)
    print(key, f"device {res:.2e} | model {rec['model_res']:.2e} | lapack {rec['lapack_res']:.2e} | bound {bound:.2e} | logabsdet {ld:.17g} "
               f"slogdet {rec['logabsdet']:.17g}")
    assert X.shape == (n, n) and X.dtype == complex and np.isfinite(X).all()
    assert res <= bound, (key, res, bound)
    assert abs(ld - rec["logabsdet"]) <= n * EPS * (max(1.0, abs(rec["logabsdet"])) if logdet_abs else abs(rec["logabsdet"])), (key, ld, rec["logabsdet"])
    assert piv.shape == (n,) and (piv >= np.arange(n)).all() and (piv < n).all()
    if n <= 70:
        assert np.array_equal(piv, cm.invert(A)[1]), key


# ---- 1. inversion: every panel variant and its edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.BATCH3)
def test_inversion_one_panel_and_its_edges_batch_of_three(ctx, n):
    """R = 1 (width 32): n = 1, 2, a tail of 31, exactly one panel, one panel and a tail of 1, sixteen full panels"""
    keys = [f"n{n}_b{b}" for b in range(3)]
    As = [tc.inversion_matrix(k) for k in keys]
    out = D.dense_invert_complex_batch(As, ctx=ctx)
    assert len(out) == 3
    for k, A, o in zip(keys, As, out):
        _check_inverse(k, A, o)


@pytest.mark.parametrize("n", tc.SINGLE)
def test_inversion_every_further_panel_variant_with_a_tail(ctx, n):
    """R = 2 .. 8 rows per thread (widths 16, 16, 8, 8, 4, 4, 4), each order with a tail panel (4096: the largest order, no tail)"""
    key = f"n{n}_b0"
    A = tc.inversion_matrix(key)
    _check_inverse(key, A, D.dense_invert_complex(A, ctx=ctx))


@pytest.mark.parametrize("n", tc.REVERSED)
def test_inversion_with_an_interchange_at_every_step(ctx, n):
    key = f"rev{n}"
    A = tc.inversion_matrix(key)
    out = D.dense_invert_complex(A, ctx=ctx)
    _check_inverse(key, A, out, logdet_abs=True)
    assert (out[1][: n // 2] == n - 1 - np.arange(n // 2)).all()


def test_real_and_imaginary_inputs_keep_their_zero_plane(ctx):
    A = tc.inversion_matrix("n33_b0").real.copy()
    X = D.dense_invert_complex(A, ctx=ctx)[0]
    assert np.array_equal(X.imag, np.zeros((33, 33)))
    assert np.linalg.norm(X.real - np.linalg.inv(A)) <= 33 * EPS * np.linalg.cond(A) * np.linalg.norm(X.real)
    Y = D.dense_invert_complex(1j * A, ctx=ctx)[0]
    assert np.array_equal(Y.real, np.zeros((33, 33)))
    assert np.linalg.norm(Y.imag + X.real) <= 33 * EPS * np.linalg.cond(A) * np.linalg.norm(X.real)          # inv(i A) = -i inv(A)


@pytest.mark.parametrize("e", [600, -600])
def test_the_pivot_reciprocal_is_safe_against_overflow(ctx, e):
    """|pivot|^2 overflows (underflows) at 2^600 (2^-600): Smith's formula does not form it"""
    A = tc.inversion_matrix("n33_b0")
    As = np.ldexp(A.real, e) + 1j * np.ldexp(A.imag, e)
    X, piv, ld = D.dense_invert_complex(As, ctx=ctx)
    assert np.isfinite(X).all()
    Xu = np.ldexp(X.real, e) + 1j * np.ldexp(X.imag, e)          # the inverse of A itself: scaling by a power of two is exact
    res, bound = tc.residual(A, Xu), tc.inversion_bound("n33_b0")
    print(f"2^{e}: residual {res:.2e}, bound {bound:.2e}")
    assert res <= bound
    ref = tc.recorded()["inversion"]["n33_b0"]["logabsdet"] + 33 * e * np.log(2.0)
    assert abs(ld - ref) <= 33 * EPS * abs(ref)


@pytest.mark.parametrize("n", [33, 513])
def test_a_member_alone_equals_the_member_in_a_batch(ctx, n):
    As = [cm.test_matrix(n, b) for b in range(3)]
    batch = D.dense_invert_complex_batch(As, ctx=ctx)
    for b in range(3):
        X, piv, ld = D.dense_invert_complex(As[b], ctx=ctx)
        assert np.array_equal(X, batch[b][0]) and np.array_equal(piv, batch[b][1]) and ld == batch[b][2]


def _raw_invert(ctx, As):
    """dre_dense_invert_complex_batched on uploaded planes -> (return code, planes after the call, status)"""
    nb = len(As)
    Ar = [ctx.upload(np.asfortranarray(A.real)) for A in As]
    Ai = [ctx.upload(np.asfortranarray(A.imag)) for A in As]
    st = np.full(nb, 9, dtype=np.int32)
    rc = ctx.lib.dre_dense_invert_complex_batched(ctx.ptr, nb, (C_.c_void_p * nb)(*[a.ptr for a in Ar]), (C_.c_void_p * nb)(*[a.ptr for a in Ai]), None,
                                                  None, st.ctypes.data_as(C_.POINTER(C_.c_int32)))
    return rc, [r.numpy() + 1j * i.numpy() for r, i in zip(Ar, Ai)], st


@pytest.mark.parametrize("bad", ["zero_column", "nan"])
def test_a_singular_member_fails_alone(ctx, bad):
    n = 70
    As = [cm.test_matrix(n, b) for b in range(3)]
    if bad == "zero_column":
        As[1][:, 40] = 0.0
    else:
        As[1][5, 17] = np.nan
    rc, planes, st = _raw_invert(ctx, As)
    assert rc == 0 and list(st) == [0, -4, 0]
    assert b"member 1" in ctx.lib.dre_batch_member_error(ctx.ptr, 1)
    assert np.array_equal(planes[1], As[1], equal_nan=True)                       # left as it came
    for b in (0, 2):
        assert np.array_equal(planes[b], D.dense_invert_complex(As[b], ctx=ctx)[0])
    with pytest.raises(D.DREError) as e:
        D.dense_invert_complex_batch(As, ctx=ctx)
    assert e.value.code == -4 and "member 1" in str(e.value)
    out = D.dense_invert_complex_batch(As, errors="return", ctx=ctx)
    assert isinstance(out[1], D.DREError) and out[1].code == -4 and np.array_equal(out[0][0], planes[0]) and np.array_equal(out[2][0], planes[2])
    with pytest.raises(D.DREError) as e:
        D.dense_invert_complex(As[1], ctx=ctx)
    assert e.value.code == -4


def test_the_c_entry_of_the_inversion_rejects_bad_arguments_before_any_launch(ctx):
    lib = ctx.lib
    a33, a34 = ctx.upload(np.zeros((33, 33), order="F")), ctx.upload(np.zeros((34, 34), order="F"))
    st = np.full(2, 9, dtype=np.int32)
    pst = st.ctypes.data_as(C_.POINTER(C_.c_int32))
    arr = lambda *h: (C_.c_void_p * len(h))(*[x.ptr for x in h])              # noqa: E731
    assert lib.dre_dense_invert_complex_batched(ctx.ptr, 0, arr(a33), arr(a33), None, None, pst) == -1
    assert lib.dre_dense_invert_complex_batched(ctx.ptr, 2, arr(a33, a33), arr(a33, a34), None, None, pst) == -1
    assert lib.dre_dense_invert_complex_batched(ctx.ptr, 1, arr(a33), arr(a34), None, None, pst) == -1
    big = ctx.upload(np.zeros((4097, 4097), order="F"))
    assert lib.dre_dense_invert_complex_batched(ctx.ptr, 1, arr(big), arr(big), None, None, pst) == -1 and b"4096" in lib.dre_last_error(ctx.ptr)
    assert (st == 9).all()


# ---- 2. transfer function ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.CASES)
def test_complex_method_against_the_frequency_record(ctx, name):
    """every case of the frequency-response record through method="complex" (index1_6: singular E)"""
    E, A, B, C = fc.system(name)
    om, Href, _, ld = fc.recorded_case(name)
    H, info = D.freq_response(E, A, B, C, om, ctx=ctx, return_info=True, method="complex")
    assert H.shape == Href.shape and H.dtype == complex
    assert info["members"] == len(om) and info["order"] == E.shape[0] and info["chunk"] * info["chunks"] >= len(om)
    d, bound = _dist(H, Href), tc.freq_bound(name)
    print(name, "device", " ".join(f"{v:.1e}" for v in d), "| model", " ".join(f"{v:.1e}" for v in tc.recorded()["freq"][name]["model_dist"]), "| lapack",
          " ".join(f"{v:.1e}" for v in ld), "| bound", " ".join(f"{v:.1e}" for v in bound))
    for k in range(len(om)):
        assert d[k] <= bound[k], (name, om[k], d[k], bound[k])
    assert np.array_equal(D.transfer_function(E, A, B, C, 1j * om, ctx=ctx), H)


@pytest.mark.parametrize("name", tc.POINT_CASES)
def test_transfer_function_at_the_recorded_complex_points(ctx, name):
    E, A, B, C = fc.system(name)
    s, Href, md, ld = tc.recorded_points(name)
    H, info = D.transfer_function(E, A, B, C, s, ctx=ctx, return_info=True)
    assert H.shape == Href.shape and info["order"] == E.shape[0] and info["members"] == 4
    d, bound = _dist(H, Href), tc.points_bound(name)
    print(name, "device", " ".join(f"{v:.1e}" for v in d), "| model", " ".join(f"{v:.1e}" for v in md), "| lapack", " ".join(f"{v:.1e}" for v in ld),
          "| bound", " ".join(f"{v:.1e}" for v in bound))
    for k in range(4):
        assert d[k] <= bound[k], (name, s[k], d[k], bound[k])
    Dm = np.arange(1.0, 1.0 + Href[0].size).reshape(Href[0].shape)
    assert np.array_equal(D.transfer_function(E, A, B, C, s, D=Dm, ctx=ctx), H + Dm)


@pytest.mark.parametrize("name", ["osc12", "pencil33", "index1_6"])
def test_zero_frequency_is_the_static_gain(ctx, name):
    E, A, B, C = fc.system(name)
    om, Href, _, _ = fc.recorded_case(name)
    assert om[0] == 0.0
    H = D.freq_response(E, A, B, C, [0.0], ctx=ctx, method="complex")[0]
    bound = tc.freq_bound(name)[0]
    assert np.array_equal(H.imag, np.zeros(H.shape))
    G = -C @ np.linalg.solve(A, B)
    assert np.linalg.norm(H.real - Href[0].real) <= bound * np.linalg.norm(Href[0])
    assert np.linalg.norm(H.real - G) <= 2 * bound * np.linalg.norm(G)


# ---- member independence, bit for bit -------------------------------------------------------------------------------------------------------
def test_order_and_company_do_not_change_a_point(ctx):
    E, A, B, C = fc.system("pencil70")
    om = np.array(fc.frequencies("pencil70") + [float(w) for w in bc.OMEGA[1::6]] + [0.25])[:17]
    s = 1j * om + np.linspace(-0.5, 0.5, 17)
    H, info = D.transfer_function(E, A, B, C, s, ctx=ctx, return_info=True)
    assert info["chunks"] == 1 and info["chunk"] == 17
    assert np.array_equal(D.transfer_function(E, A, B, C, s[::-1], ctx=ctx), H[::-1])
    for k in (0, 5, 16):
        assert np.array_equal(D.transfer_function(E, A, B, C, s[k:k + 1], ctx=ctx)[0], H[k])


@pytest.mark.parametrize("chunk", [1, 3])
def test_the_chunk_does_not_change_a_point(ctx, chunk):
    E, A, B, C = fc.system("osc12")
    om = [0.0, 0.3, 2.0, 2.0001, 11.0, 0.7, 40.0]
    H = D.freq_response(E, A, B, C, om, ctx=ctx, method="complex")
    Hc, info = D.freq_response(E, A, B, C, om, chunk=chunk, ctx=ctx, return_info=True, method="complex")
    assert info["chunk"] == chunk and info["chunks"] == -(-7 // chunk)
    assert np.array_equal(Hc, H)


@pytest.mark.parametrize("chunk", [None, 1, 4])
def test_ensemble_members_equal_the_single_calls(ctx, chunk):
    E, A, B, C = fc.system("pencil33")
    rng = np.random.default_rng(3)
    systems = [(E, A, B, C), (E, A * 1.25, B[:, ::-1].copy(), C), (E + 0.01 * rng.standard_normal(E.shape), A, B, 2.0 * C)]
    s = np.array([0.0, 1e-3j, 0.1 + 0.5j, -0.2 + 30.0j, 1e3j])
    H, info = D.transfer_function_batch(systems, s, chunk=chunk, ctx=ctx, return_info=True)
    assert H.shape == (3, 5, C.shape[0], B.shape[1]) and info["members"] == 15
    if chunk == 4:
        assert info["chunks"] == 4          # chunks 1 and 2 hold points of two systems each
    for i, sys_ in enumerate(systems):
        assert np.array_equal(H[i], D.transfer_function(*sys_, s, ctx=ctx)), i
    Hf = D.freq_response_batch(systems, [0.5, 30.0], chunk=chunk, ctx=ctx, method="complex")
    for i, sys_ in enumerate(systems):
        assert np.array_equal(Hf[i], D.freq_response(*sys_, [0.5, 30.0], ctx=ctx, method="complex")), i


# ---- failures -----------------------------------------------------------------------------------------------------------------------------
def _singular_at_zero():
    """a zero row and column in A: s E - A is singular at s = 0 with an exactly zero pivot column, regular at s = i"""
    E, A, B, C = (np.array(M) for M in fc.system("one_panel8"))
    A[3, :] = 0.0
    A[:, 3] = 0.0
    E = np.eye(8)
    return E, A, B, C


def test_a_point_on_a_pole_fails_alone(ctx):
    E, A, B, C = _singular_at_zero()
    with pytest.raises(D.DREError) as e:
        D.freq_response(E, A, B, C, [0.0, 1.0], ctx=ctx, method="complex")
    assert e.value.code == -4 and "point 0" in str(e.value) and "singular" in str(e.value)
    H, errs = D.freq_response(E, A, B, C, [0.0, 1.0], errors="return", ctx=ctx, method="complex")
    assert isinstance(errs[0], D.DREError) and errs[0].code == -4 and errs[1] is None
    assert np.isnan(H[0].real).all() and np.isnan(H[0].imag).all()
    Href = C @ np.linalg.solve(1j * E - A, B.astype(complex))
    assert np.linalg.norm(H[1] - Href) <= 10.0 * 8 * EPS * np.linalg.cond(1j * E - A) * np.linalg.norm(Href)
    assert np.array_equal(H[1], D.transfer_function(E, A, B, C, [1j], ctx=ctx)[0])
    S, errs = D.sigma_response(E, A, B, C, [0.0, 1.0], errors="return", ctx=ctx, method="complex")
    assert np.isnan(S[0]).all() and np.array_equal(S[1], np.linalg.svd(H[1], compute_uv=False)) and errs[0].code == -4
    # a NaN in the system: every point of that system, and only that system
    An = A.copy()
    An[0, 0] = np.nan
    good = fc.system("one_panel8")
    s = [0.5j, 0.3 + 1.0j]
    Hb, eb = D.transfer_function_batch([good, (E, An, B, C)], s, errors="return", ctx=ctx)
    assert eb[0] == [None, None] and [x.code for x in eb[1]] == [-4, -4] and "system 1" in str(eb[1][1])
    assert np.isnan(Hb[1]).all() and np.array_equal(Hb[0], D.transfer_function(*good, s, ctx=ctx))
    with pytest.raises(D.DREError) as e:
        D.transfer_function_batch([good, (E, An, B, C)], s, ctx=ctx)
    assert e.value.code == -4
    # the context lives on
    assert np.isfinite(D.transfer_function(*good, [0.0], ctx=ctx)).all()


def test_the_c_entry_rejects_bad_arguments_before_any_launch(ctx):
    E, A, B, C = (ctx.upload(np.asfortranarray(M)) for M in fc.system("one_panel8"))
    lib = ctx.lib
    pd, pi32 = C_.POINTER(C_.c_double), C_.POINTER(C_.c_int32)
    re, im, st = np.full(6 * 4, 7.0), np.full(6 * 4, 7.0), np.full(4, 9, dtype=np.int32)

    def call(Eh, Ah, Bh, Ch, s, K=None, chunk=0):
        s = np.array(s, dtype=complex)
        sr, si = np.ascontiguousarray(s.real), np.ascontiguousarray(s.imag)
        return lib.dre_transfer_eval(ctx.ptr, Eh.ptr, Ah.ptr, Bh.ptr, Ch.ptr, len(s) if K is None else K, sr.ctypes.data_as(pd), si.ctypes.data_as(pd),
                                     chunk, re.ctypes.data_as(pd), im.ctypes.data_as(pd), st.ctypes.data_as(pi32), None)
    assert call(E, A, B, C, [1.0, complex(np.nan, 0.0)]) == -1 and b"not finite" in lib.dre_last_error(ctx.ptr)
    assert call(E, A, B, C, [complex(0.0, np.inf)]) == -1
    assert call(E, A, B, C, [1.0], K=0) == -1 and b"K >= 1" in lib.dre_last_error(ctx.ptr)
    assert call(E, A, B, C, [1.0], chunk=-1) == -1 and call(E, A, B, C, [1.0], chunk=65536) == -1
    assert call(E, A, C, C, [1.0]) == -1 and call(E, A, B, B, [1.0]) == -1 and call(B, A, B, C, [1.0]) == -1 and call(E, C, B, C, [1.0]) == -1
    # n = 4097: DRE_ERR_INVALID with nothing launched
    big = ctx.upload(np.zeros((4097, 4097), order="F"))
    assert call(big, big, ctx.upload(np.zeros((4097, 1))), ctx.upload(np.zeros((1, 4097))), [1.0]) == -1 and b"n <= 4096" in lib.dre_last_error(ctx.ptr)
    # nothing was written
    assert (re == 7.0).all() and (im == 7.0).all() and (st == 9).all()
    # and the call works afterwards, with info
    info = (C_.c_int64 * 2)()
    s = np.array([0.3 + 1.0j, -0.2 + 0.5j])
    sr, si = np.ascontiguousarray(s.real), np.ascontiguousarray(s.imag)
    assert lib.dre_transfer_eval(ctx.ptr, E.ptr, A.ptr, B.ptr, C.ptr, 2, sr.ctypes.data_as(pd), si.ctypes.data_as(pd), 0, re.ctypes.data_as(pd),
                                 im.ctypes.data_as(pd), st.ctypes.data_as(pi32), info) == 0
    assert list(info) == [2, 1] and (st[:2] == 0).all()
    _, Href, _, _ = tc.recorded_points("one_panel8")
    H = (re[:12] + 1j * im[:12]).reshape(2, 2, 3).transpose(0, 2, 1)
    assert (_dist(H, Href[:2]) <= tc.points_bound("one_panel8")[:2]).all()


def test_a_forced_chunk_that_does_not_fit_is_an_allocation_error(ctx):
    """65535 members of n = 1024 would hold 65535 x 2 x 1024^2 doubles (1 TiB): DRE_ERR_ALLOC before any kernel"""
    n = 1024
    E = ctx.upload(np.asfortranarray(np.eye(n)))
    A = ctx.upload(np.asfortranarray(-np.eye(n)))
    B, Cm = ctx.upload(np.ones((n, 1))), ctx.upload(np.ones((1, n)))
    K = 65535
    pd, pi32 = C_.POINTER(C_.c_double), C_.POINTER(C_.c_int32)
    sr, si = np.zeros(K), np.ones(K)
    re, im, st = np.full(K, 7.0), np.full(K, 7.0), np.full(K, 9, dtype=np.int32)
    rc = ctx.lib.dre_transfer_eval(ctx.ptr, E.ptr, A.ptr, B.ptr, Cm.ptr, K, sr.ctypes.data_as(pd), si.ctypes.data_as(pd), K, re.ctypes.data_as(pd),
                                   im.ctypes.data_as(pd), st.ctypes.data_as(pi32), None)
    assert rc == -3 and b"MiB" in ctx.lib.dre_last_error(ctx.ptr)          # DRE_ERR_ALLOC
    assert (re == 7.0).all() and (st == 9).all()
    assert np.isfinite(D.transfer_function(*fc.system("one_panel8"), [1j], ctx=ctx)).all()


# ---- beyond the embedding's limit -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.LARGE_N)
def test_beyond_the_embeddings_limit(ctx, n):
    """n = 2049 (the first order the embedding refuses) and n = 4096 (the panel's limit), m = q = 1, K = 2, against LAPACK's complex solve within
    2 n eps cond_1(i w E - A)"""
    E, A, B, C = tc.large_system(n)
    Href, bound = tc.recorded_large(n)
    H, info = D.freq_response(E, A, B, C, tc.LARGE_OMEGA, ctx=ctx, return_info=True, method="complex")
    d = _dist(H, Href)
    print(f"n={n}: device", " ".join(f"{v:.2e}" for v in d), "| bound", " ".join(f"{v:.2e}" for v in bound), "| chunk", info["chunk"])
    assert info["order"] == n and (d <= bound).all()
    with pytest.raises(ValueError, match="n <= 2048"):
        D.freq_response(E, A, B, C, tc.LARGE_OMEGA, ctx=ctx)


# ---- the guarantee, end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,r", [(33, 8), (70, 12)])
def test_bt_error_with_the_complex_method_reproduces_the_embeddings(ctx, n, r):
    E, A, Bm, Cm = bc.system(n)
    rom = D.balanced_truncation(E, A, Bm, Cm, order=r, ctx=ctx)
    res = D.bt_error(E, A, Bm, Cm, rom, bc.OMEGA, ctx=ctx, method="complex")
    ref = D.bt_error(E, A, Bm, Cm, rom, bc.OMEGA, ctx=ctx)
    print(f"n={n} r={r}: complex {res['max_error']:.16e}, embedding {ref['max_error']:.16e}, ratio {res['ratio']:.4f}")
    assert abs(res["max_error"] - ref["max_error"]) <= 1e-10 * ref["max_error"]
    assert res["ratio"] >= 1.0 and res["bound"] == ref["bound"]
    assert np.array_equal(rom.freq_response(bc.OMEGA[:3], ctx=ctx, method="complex"), D.transfer_function(np.eye(r), rom.Ar, rom.Br, rom.Cr, 1j * bc.OMEGA[:3], ctx=ctx))
