"""Every entry point of the f64 MFMA GEMM family (csrc/gemm.hip, gemm_sym_update of csrc/dense.hip) on its own, through dre_gemm_probe, at the
smallest shapes at which each path changes behaviour.  Every case runs twice (tests/_gemm_probe.py): bit for bit on integer operands, and
against np.longdouble within the derived componentwise bound (K + 2) eps (|alpha| |op A| |op B| + |beta| |C|).  Operands are views inside
larger buffers: NaN around the inputs, a sentinel around every output that must come back bit-identical."""
import numpy as np
import pytest

import _gemm_probe as G
from _gemm_probe import GEMM, THIN, STRIDED, BATCHED, ROWS, ZRED, SYM, ERR_INVALID, LD, EPS, Region, op, options, probe

pytestmark = pytest.mark.gpu

PASS = pytest.mark.parametrize("P", G.PASSES, ids=lambda p: p.name)
TRANSPOSES = ((0, 0), (1, 0), (0, 1), (1, 1))
AB = ((1.0, -2.0), (-2.0, 0.5), (0.5, 1.0), (1.0, 0.0), (-2.0, 0.0), (0.5, 0.0))      # (alpha, beta); beta = 0 runs over a NaN-filled C


def _seed(*v):
    return np.random.default_rng([int(x) for x in v])


def _operands(ctx, P, rng, tA, tB, M, N, K, beta):
    A = P.gen(rng, (K, M) if tA else (M, K))          # asymmetric operands catch swapped lane maps
    B = P.gen(rng, (N, K) if tB else (K, N))
    C0 = P.gen(rng, (M, N))
    rA = Region(ctx, *A.shape, data=A)
    rB = Region(ctx, *B.shape, data=B, off=3)
    rC = Region(ctx, M, N, data=C0 if beta != 0.0 else np.full((M, N), np.nan), fill="sentinel")      # beta = 0: the old C is NaN and must not show
    return A, B, C0, rA, rB, rC


def _gemm_once(ctx, P, seed, tA, tB, M, N, K, alpha, beta, opts=None, check=True):
    A, B, C0, rA, rB, rC = _operands(ctx, P, _seed(*seed), tA, tB, M, N, K, beta)
    rc, splits = probe(ctx, GEMM, tA, tB, alpha, rA, rB, beta, rC, opts)
    what = f"gemm {P.name} tA={tA} tB={tB} M={M} N={N} K={K} alpha={alpha} beta={beta} splits={splits}"
    assert rc == 0, what
    out = rC.result(what)[0]
    if check:
        P.check(out, alpha, op(A, tA), op(B, tB), beta, C0, what)
    return out, splits


# ---- gemm ------------------------------------------------------------------------------------------------------------------------------
GEMM_K = (0, 1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 520, 777, 1000, 2100)
GEMM_MN = ((1, 1), (15, 17), (16, 64), (17, 15), (63, 65), (64, 16), (65, 63), (130, 1), (1, 130), (130, 130), (64, 64), (16, 130), (130, 17))


@PASS
@pytest.mark.parametrize("ik", range(len(GEMM_K)), ids=lambda i: f"K{GEMM_K[i]}")
def test_gemm_all_transposes(ctx, P, ik):
    K = GEMM_K[ik]
    for it, (tA, tB) in enumerate(TRANSPOSES):
        M, N = GEMM_MN[(4 * ik + it) % len(GEMM_MN)]
        alpha, beta = AB[(ik + it) % len(AB)]
        _gemm_once(ctx, P, (1, ik, it), tA, tB, M, N, K, alpha, beta)      # K = 0: beta C, or zeros for beta = 0 (the references say so too)


def test_gemm_split_counts_reach_every_branch_of_the_reduce(ctx):
    """k_gemm_reduce sums slabs in groups of 8, then of 4, then one by one: the K list must make the host choose split counts of every class."""
    seen = set()
    for ik, K in enumerate(GEMM_K):
        tA, tB = TRANSPOSES[ik % 4]
        _, s = _gemm_once(ctx, G.Exact, (2, ik), tA, tB, 17, 15, K, -2.0, 0.5)
        seen.add(s)
    assert 1 in seen, seen
    assert any(2 <= s <= 3 for s in seen), seen
    assert any(4 <= s <= 7 for s in seen), seen
    assert any(s >= 8 and 1 <= s % 8 <= 3 for s in seen), seen
    assert any(s >= 12 for s in seen), seen


SWZ_SHAPES = ((130, 65, 200), (65, 130, 520), (64, 64, 129), (130, 130, 64), (65, 64, 1000), (130, 200, 300))


@PASS
def test_gemm_swizzle_2_moves_the_assignment_only(ctx, P):
    """gemm_swizzle = 2 swizzles every launch: same tiling, other workgroups, so the result is bit-identical to launch order."""
    grids = []
    for i, (M, N, K) in enumerate(SWZ_SHAPES):
        for it, (tA, tB) in enumerate(TRANSPOSES):
            alpha, beta = AB[(i + it) % len(AB)]
            outs = []
            for swz in (0, 2):
                ctx.set_option("gemm_swizzle", swz)
                out, s = _gemm_once(ctx, P, (3, i, it), tA, tB, M, N, K, alpha, beta, check=(swz == 2))
                outs.append(out)
            assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), (M, N, K, tA, tB)
            grids.append(((M + 63) // 64, (N + 63) // 64, s))
    assert any((gx * gy * gz) % 8 != 0 for gx, gy, gz in grids), grids
    assert any((gx * gy * gz) % 8 != 0 and gx * gy * gz > 8 for gx, gy, gz in grids), grids
    assert any(gx <= gy and gz > 1 for gx, gy, gz in grids) and any(gx > gy and gz > 1 for gx, gy, gz in grids), grids
    assert any(gx < gy for gx, gy, gz in grids), grids


# ---- tile_sumsq ------------------------------------------------------------------------------------------------------------------------
@PASS
@pytest.mark.parametrize("K", (1, 32, 64))
@pytest.mark.parametrize("swz", (0, 2))
def test_gemm_tile_sumsq(ctx, P, K, swz):
    ctx.set_option("gemm_swizzle", swz)
    for i, (M, N) in enumerate(((37, 50), (100, 33), (130, 100))):          # 1, 2 and 6 tiles, ragged edges
        tA, tB = TRANSPOSES[(i + K) % 4]
        alpha, beta = AB[(i + K // 32) % len(AB)]
        A, B, C0, rA, rB, rC = _operands(ctx, P, _seed(4, K, i), tA, tB, M, N, K, beta)
        gx, gy = (M + 63) // 64, (N + 63) // 64
        rS = Region(ctx, gx * gy, 1, fill="sentinel", ld=gx * gy, off=0, tail=3)
        rc, splits = probe(ctx, GEMM, tA, tB, alpha, rA, rB, beta, rC, options(tile_sumsq=rS.dev))
        what = f"tile_sumsq {P.name} {M}x{N}x{K}"
        assert rc == 0 and splits == 1, what
        out = rC.result(what)[0]
        P.check(out, alpha, op(A, tA), op(B, tB), beta, C0, what)
        ss = rS.result(what)[0][:, 0]
        for by in range(gy):
            for bx in range(gx):
                tile = out[64 * bx:64 * bx + 64, 64 * by:64 * by + 64].astype(LD)      # the DOWNLOADED C tile
                want = (tile * tile).sum()
                got = ss[bx + gx * by]
                if P is G.Exact:
                    assert got == float(want), (what, bx, by)
                else:
                    assert abs(LD(got) - want) <= (4096 + 8) * EPS * want, (what, bx, by, float(abs(LD(got) - want) / want))


def test_gemm_tile_sumsq_refuses_a_split_k(ctx):
    A, B, C0, rA, rB, rC = _operands(ctx, G.Exact, _seed(5), 0, 0, 37, 50, 65, 1.0)
    rS = Region(ctx, 1, 1, fill="sentinel", ld=1, off=0, tail=3)
    rc, _ = probe(ctx, GEMM, 0, 0, 1.0, rA, rB, 1.0, rC, options(tile_sumsq=rS.dev))
    assert rc == ERR_INVALID
    rC.assert_untouched(); rS.assert_untouched()


# ---- the probe's own bounds check, on the device path (no launch may follow a refusal) ----------------------------------------------------
def test_probe_refuses_views_outside_their_buffers(ctx):
    A, B, C0, rA, rB, rC = _operands(ctx, G.Exact, _seed(6), 0, 0, 20, 10, 8, 1.0)
    n = rC.host.size
    bad = [
        (rA.view(off=rA.host.size - 10), rB, rC, None),                  # A runs off the end
        (rA, rB.view(ld=7), rC, None),                                    # ld below the row count
        (rA, rB, rC.view(off=n - (9 * rC.ld + 20) + 1), None),            # C one element too far
        (rA, rB, rC.view(off=-1), None),
        (rA, rB, rC.view(rows=19), None),                                 # shape mismatch
        (rA, rB, None, None),
        (rA, rB, rC, options(batch=2)),                                   # gemm takes no batch
        (rA, rB, rC, options(use_count=1, iters=1, nmax=1, per=1)),       # ... and no device-side count
    ]
    for a, b, c, o in bad:
        assert probe(ctx, GEMM, 0, 0, 1.0, a, b, 1.0, c, o)[0] == ERR_INVALID
    assert probe(ctx, 7, 0, 0, 1.0, rA, rB, 1.0, rC)[0] == ERR_INVALID
    # a stack whose last member does not fit; a rowmap entry outside C
    assert probe(ctx, STRIDED, 0, 0, 1.0, rA, rB, 1.0, rC, options(batch=2, stride_a=0, stride_b=0, stride_c=rC.stride))[0] == ERR_INVALID
    assert probe(ctx, ROWS, 0, 0, 1.0, rA, rB, 0.0, rC, options(rowmap=list(range(19)) + [20]))[0] == ERR_INVALID
    assert probe(ctx, ZRED, 0, 0, 1.0, rA, rB, 0.0, rC, options(batch=3, cz=rC.stride))[0] == ERR_INVALID
    small = Region(ctx, 1, 1, fill="sentinel", ld=1, off=0, tail=0)                      # two tiles, room for one sum
    A2, B2, C2, rA2, rB2, rC2 = _operands(ctx, G.Exact, _seed(6, 1), 0, 0, 70, 10, 8, 1.0)
    assert probe(ctx, GEMM, 0, 0, 1.0, rA2, rB2, 1.0, rC2, options(tile_sumsq=small.dev))[0] == ERR_INVALID
    rC2.assert_untouched(); small.assert_untouched()
    rC.assert_untouched()
    assert probe(ctx, GEMM, 0, 0, 1.0, rA, rB, 1.0, rC)[0] == 0          # and the well-formed call goes through


# ---- done flag -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", (GEMM, THIN, ROWS, ZRED), ids=("gemm", "thin", "rows", "z"))
def test_done_flag_leaves_every_output_untouched(ctx, kind):
    for K in (40, 777):                                                   # one slab and nine
        M, N = 33, 17
        A, B, C0, rA, rB, rC = _operands(ctx, G.Exact, _seed(7, kind, K), 0, 0, M, N, K, 1.0)
        o = options(use_done=1, done=1, rowmap=list(range(M))[::-1]) if kind in (ROWS, ZRED) else options(use_done=1, done=1)
        rc, _ = probe(ctx, kind, 0, 0, 1.0, rA, rB, 1.0, rC, o)
        assert rc == 0
        rC.assert_untouched(f"kind {kind} K {K}")
        o.done = 0                                                        # the same call with the flag down writes
        assert probe(ctx, kind, 0, 0, 1.0, rA, rB, 1.0, rC, o)[0] == 0
        assert not np.array_equal(rC.download().view(np.uint64), rC.host.view(np.uint64))


# ---- DevCount on gemm_partials ---------------------------------------------------------------------------------------------------------
@PASS
@pytest.mark.parametrize("per,nmax,tA,tB", ((1, 200, 0, 0), (3, 70, 1, 0), (3, 70, 0, 1), (1, 200, 1, 1)))
def test_gemm_partials_device_count_shortens_k(ctx, P, per, nmax, tA, tB):
    """The host sizes the slabs from the full K = per * nmax; the device shortens K to per * clamp(iters - base, 0, nmax).  Operand entries
    beyond the shortened K are NaN: they must not be read.  A count of 0 gives exact zeros, not stale slabs."""
    M, N, K, base = 70, 33, per * nmax, 5
    rng = _seed(8, per, tA, tB)
    rowmap = rng.permutation(M + 6)[:M]
    for cnt in (-2, 0, 37, nmax, nmax + 9):
        ke = per * min(max(cnt, 0), nmax)
        A = P.gen(rng, (K, M) if tA else (M, K)); B = P.gen(rng, (N, K) if tB else (K, N))
        Ah, Bh = A.copy(), B.copy()
        (Ah[ke:, :] if tA else Ah[:, ke:])[...] = np.nan
        (Bh[:, ke:] if tB else Bh[ke:, :])[...] = np.nan
        rA, rB = Region(ctx, *A.shape, data=Ah), Region(ctx, *B.shape, data=Bh)
        rC = Region(ctx, M + 6, N, fill="sentinel")
        rc, splits = probe(ctx, ROWS, tA, tB, 1.0, rA, rB, 0.0, rC, options(rowmap=rowmap, use_count=1, iters=base + cnt, base=base, nmax=nmax, per=per))
        what = f"partials count {cnt} per {per} tA={tA} tB={tB} splits={splits}"
        assert rc == 0 and splits == 3, what                              # (ke = 37, 111 end inside a 96-wide K-chunk)
        got = rC.result(what)[0]
        keep = np.ones(M + 6, dtype=bool); keep[rowmap] = False
        assert np.array_equal(got[keep].view(np.uint64), rC.host[rC.idx][0][keep].view(np.uint64)), what      # rows outside the map
        Ao, Bo = op(A, tA)[:, :ke], op(B, tB)[:ke, :]
        P.check(got[rowmap], 1.0, Ao, Bo, 0.0, None, what)
        if ke == 0:
            assert not got[rowmap].any(), what


# ---- gemm_thin -------------------------------------------------------------------------------------------------------------------------
THIN_K = (1, 2, 3, 4, 5, 13, 16, 17, 95, 96, 97, 383, 384, 385, 389, 2048, 5177)
THIN_MN = ((1, 1), (15, 33), (16, 16), (17, 15), (33, 17), (1, 33), (33, 1), (16, 17), (15, 16))


@PASS
@pytest.mark.parametrize("ik", range(len(THIN_K)), ids=lambda i: f"K{THIN_K[i]}")
def test_gemm_thin(ctx, P, ik):
    K = THIN_K[ik]
    for tA in (0, 1):
        for j in range(2):
            M, N = THIN_MN[(3 * ik + 2 * tA + j) % len(THIN_MN)]
            alpha, beta = AB[(ik + tA + 3 * j) % len(AB)]                 # j = 0 / 1 alternate between beta != 0 and beta = 0 over NaN
            A, B, C0, rA, rB, rC = _operands(ctx, P, _seed(9, ik, tA, j), tA, 0, M, N, K, beta)
            rc, _ = probe(ctx, THIN, tA, 0, alpha, rA, rB, beta, rC)
            what = f"thin {P.name} tA={tA} {M}x{N}x{K} alpha={alpha} beta={beta}"
            assert rc == 0, what
            P.check(rC.result(what)[0], alpha, op(A, tA), B, beta, C0, what)


def test_gemm_thin_covers_both_beta_forms_at_every_k():
    for ik in range(len(THIN_K)):
        for tA in (0, 1):
            betas = {AB[(ik + tA + 3 * j) % len(AB)][1] == 0.0 for j in range(2)}
            assert betas == {True, False}, (ik, tA)


def test_gemm_thin_refuses_an_empty_inner_dimension(ctx):
    A, B, C0, rA, rB, rC = _operands(ctx, G.Exact, _seed(10), 0, 0, 17, 15, 0, 1.0)
    assert probe(ctx, THIN, 0, 0, 1.0, rA, rB, 1.0, rC)[0] == ERR_INVALID
    rC.assert_untouched()


# ---- gemm_strided ----------------------------------------------------------------------------------------------------------------------
STRIDED_SHAPES = ((65, 31, 33), (64, 64, 32), (17, 130, 64), (1, 1, 1), (63, 33, 65), (130, 17, 31))
COEF = ((1.0, -2.0), (0.0, 0.5), (-2.0, 0.0), (0.5, 1.0), (1.0, 0.5))


def _strided(ctx, P, seed, batch, tA, tB, M, N, K, mask=None, coef=None, alpha=1.0, beta=-2.0, members=None):
    """One gemm_strided call on a stack; returns (result (batch, M, N), expected-per-member checker inputs).  members: run only these members
    of the same data, each as a batch of 1 (for the batch-independence check)."""
    rng = _seed(*seed)
    sa = (K, M) if tA else (M, K)
    sb = (N, K) if tB else (K, N)
    A = P.gen(rng, (batch,) + sa); B = P.gen(rng, (batch,) + sb); C0 = P.gen(rng, (batch, M, N))
    ab = [(coef[b] if coef is not None else (alpha, beta)) for b in range(batch)]
    Cin = C0.copy()
    for b in range(batch):
        if ab[b][1] == 0.0 and (mask is None or mask[b]):
            Cin[b] = np.nan                                               # beta_b = 0 runs over NaN
    rA = Region(ctx, *sa, count=batch, data=A, ld=2 * sa[0])              # ld = 2 rows, as the Hamiltonian blocks have
    rB = Region(ctx, *sb, count=batch, data=B)
    rC = Region(ctx, M, N, count=batch, data=Cin, fill="sentinel")        # member stride larger than M * N, as Pstore has
    assert rC.stride > M * N
    kw = dict(batch=batch, stride_a=rA.stride, stride_b=rB.stride, stride_c=rC.stride)
    if mask is not None:
        kw["member_on"] = mask
    if coef is not None:
        kw["coef"] = [x for b in range(batch) for x in (ab[b][0], ab[b][1], 99.0)]; kw["coef_stride"] = 3
        alpha, beta = 7.0, 9.0                                            # the scalar arguments must be ignored
    if members is None:
        rc, _ = probe(ctx, STRIDED, tA, tB, alpha, rA, rB, beta, rC, options(**kw))
        assert rc == 0
    else:
        for b in members:
            kw1 = dict(kw, batch=1)
            if mask is not None: kw1["member_on"] = [mask[b]]
            if coef is not None: kw1["coef"] = kw["coef"][3 * b:3 * b + 3]
            rc, _ = probe(ctx, STRIDED, tA, tB, alpha, rA.view(b), rB.view(b), beta, rC.view(b), options(**kw1))
            assert rc == 0
    return rC.result("strided"), A, B, C0, Cin, ab


@PASS
@pytest.mark.parametrize("batch", (1, 3, 5))
def test_gemm_strided_masks_and_member_coefficients(ctx, P, batch):
    for i, (M, N, K) in enumerate(STRIDED_SHAPES):
        tA, tB = TRANSPOSES[(i + batch) % 4]
        for variant in range(3):
            mask = None; coef = None
            if variant == 1:
                mask = [(b + i) % 2 for b in range(batch)] if batch > 1 else [0]          # batch 5, even i: drops the first, the middle and the last member
            if variant == 2:
                coef = [COEF[(b + i) % len(COEF)] for b in range(batch)]
                mask = [0 if (batch == 5 and b == 2) else 1 for b in range(batch)]
            alpha, beta = AB[(i + variant) % 3]
            out, A, B, C0, Cin, ab = _strided(ctx, P, (11, batch, i, variant), batch, tA, tB, M, N, K, mask, coef, alpha, beta)
            for b in range(batch):
                what = f"strided {P.name} batch {batch} member {b} {M}x{N}x{K} tA={tA} tB={tB} variant {variant}"
                if mask is not None and not mask[b]:
                    assert np.array_equal(out[b].view(np.uint64), Cin[b].view(np.uint64)), what + ": a masked member was written"
                else:
                    P.check(out[b], ab[b][0], op(A[b], tA), op(B[b], tB), ab[b][1], C0[b], what)


def test_gemm_strided_mask_patterns_drop_first_middle_and_last():
    masks = [[(b + i) % 2 for b in range(5)] for i in range(len(STRIDED_SHAPES))]
    assert [0, 1, 0, 1, 0] in masks and [1, 0, 1, 0, 1] in masks
    coefs = {COEF[(b + i) % len(COEF)] for i in range(len(STRIDED_SHAPES)) for b in range(5)}
    assert any(a == 0.0 and b != 0.0 for a, b in coefs) and any(a != 0.0 and b == 0.0 for a, b in coefs)


@PASS
def test_gemm_strided_member_does_not_depend_on_the_batch(ctx, P):
    for i, (M, N, K) in enumerate(STRIDED_SHAPES):
        tA, tB = TRANSPOSES[i % 4]
        coef = [COEF[(b + i) % len(COEF)] for b in range(5)]
        full = _strided(ctx, P, (12, i), 5, tA, tB, M, N, K, None, coef)[0]
        alone = _strided(ctx, P, (12, i), 5, tA, tB, M, N, K, None, coef, members=range(5))[0]
        assert np.array_equal(full.view(np.uint64), alone.view(np.uint64)), (M, N, K)


# ---- gemm_batched ----------------------------------------------------------------------------------------------------------------------
BM, BN, BK = (1, 63, 64, 65, 100, 17, 130), (65, 64, 1, 63, 33), (1, 7, 40)


def _batched(ctx, P, nprod, count=None, zero_n_at=None):
    rng = _seed(13, nprod)
    prods, recs = [], []
    for i in range(nprod):
        M, N, K = BM[i % len(BM)], BN[i % len(BN)], BK[i % len(BK)]
        if i == zero_n_at:
            N = 0
        A, B = P.gen(rng, (M, K)), P.gen(rng, (K, N))
        alpha = (1.0, -2.0, 0.5)[i % 3]
        rA, rB = Region(ctx, M, K, data=A), Region(ctx, K, N, data=B, off=5)
        rC = Region(ctx, M, N, data=np.full((M, N), np.nan), fill="sentinel")
        rD = Region(ctx, M, K, fill="sentinel", ld=M + 4) if (i % 3 == 0 or i == zero_n_at) else None        # ldcopy > M
        prods.append(G.ProductC(rA.view(), rB.view(), rC.view(), rD.view() if rD else G.ViewC(), alpha))
        recs.append((A, B, alpha, rC, rD, (M, N, K), rA, rB))          # (the regions live as long as the record)
    o = options(prod=prods) if count is None else options(prod=prods, use_count=1, iters=count[0], base=count[1], nmax=count[2], per=1)
    rc, _ = probe(ctx, BATCHED, 0, 0, 0.0, None, None, 0.0, None, o)
    return rc, recs


def _check_batched(P, recs, formed):
    for i, (A, B, alpha, rC, rD, shape, _, _) in enumerate(recs):
        what = f"batched {P.name} product {i} of {len(recs)} {shape}"
        if i < formed:
            P.check(rC.result(what)[0], alpha, A, B, 0.0, None, what)
            if rD is not None:
                assert np.array_equal(rD.result(what)[0], A), what + ": copy_dst"
        else:
            rC.assert_untouched(what)
            if rD is not None:
                rD.assert_untouched(what)


@PASS
@pytest.mark.parametrize("nprod", (1, 48, 49))
def test_gemm_batched_both_kernels(ctx, P, nprod):
    """<= 48 products travel as kernel arguments, 49 as a descriptor array.  Product 4 of the long lists has N = 0 and a copy_dst: the copy happens."""
    rc, recs = _batched(ctx, P, nprod, zero_n_at=4 if nprod > 1 else None)
    assert rc == 0
    _check_batched(P, recs, nprod)
    if nprod > 1:
        assert recs[4][5][1] == 0 and recs[4][4] is not None
        assert any(r[4] is not None for r in recs) and any(r[4] is None for r in recs)


@PASS
def test_gemm_batched_single_product_without_columns_still_copies(ctx, P):
    rc, recs = _batched(ctx, P, 1, zero_n_at=0)
    assert rc == 0
    _check_batched(P, recs, 1)


@PASS
def test_gemm_batched_device_count_cuts_the_list(ctx, P):
    rc, recs = _batched(ctx, P, 48, count=(25, 5, 48), zero_n_at=4)       # clamp(25 - 5, 0, 48) = 20 products are formed
    assert rc == 0
    _check_batched(P, recs, 20)
    rc, recs = _batched(ctx, P, 48, count=(60, 5, 30), zero_n_at=4)       # the count stops at nmax
    assert rc == 0
    _check_batched(P, recs, 30)


def test_gemm_batched_refuses_a_device_count_on_49_products(ctx):
    rc, recs = _batched(ctx, G.Exact, 49, count=(25, 5, 49))
    assert rc == ERR_INVALID
    _check_batched(G.Exact, recs, 0)


# ---- gemm_partials + gemm_reduce_rows --------------------------------------------------------------------------------------------------
@PASS
@pytest.mark.parametrize("K,want_splits", ((40, 1), (777, 9), (1000, 11), (2100, 22)))
def test_gemm_partials_reduce_rows_scatter(ctx, P, K, want_splits):
    """rowmap: a permutation into a taller C with ldc > its rows; 9 = one group of 8 + a tail of 1, 11 = 8 + 3, 22 = 2 x 8 + 6."""
    for it, (tA, tB) in enumerate(TRANSPOSES):
        M, N = ((33, 17), (17, 33), (64, 15), (1, 16))[it]
        rng = _seed(14, K, it)
        A = P.gen(rng, (K, M) if tA else (M, K)); B = P.gen(rng, (N, K) if tB else (K, N))
        rowmap = rng.permutation(M + 6)[:M]
        if np.array_equal(rowmap, np.arange(M)):
            rowmap = rowmap + 6                                           # (M = 1 can draw the identity)
        rA, rB, rC = Region(ctx, *A.shape, data=A), Region(ctx, *B.shape, data=B), Region(ctx, M + 6, N, fill="sentinel")
        ctx.set_option("gemm_swizzle", 2 if it % 2 else 0)
        rc, splits = probe(ctx, ROWS, tA, tB, 1.0, rA, rB, 0.0, rC, options(rowmap=rowmap))
        what = f"rows {P.name} {M}x{N}x{K} tA={tA} tB={tB}"
        assert rc == 0 and splits == want_splits, (what, splits)
        got = rC.result(what)[0]
        keep = np.ones(M + 6, dtype=bool); keep[rowmap] = False
        assert np.array_equal(got[keep].view(np.uint64), rC.host[rC.idx][0][keep].view(np.uint64)), what
        P.check(got[rowmap], 1.0, op(A, tA), op(B, tB), 0.0, None, what)


# ---- gemm_partials_z + gemm_reduce_z ---------------------------------------------------------------------------------------------------
@PASS
@pytest.mark.parametrize("nz", (1, 3, 16))
def test_gemm_partials_z_reduce_z(ctx, P, nz):
    seen = set()
    for tA in (0, 1):
        for mapped in (0, 1):
            for K in (40, 777):
                M, N = (33, 17) if tA else (65, 15)
                rng = _seed(15, nz, tA, mapped, K)
                sa = (K, M) if tA else (M, K)
                A = P.gen(rng, (nz,) + sa); B = P.gen(rng, (nz, K, N))
                rows_c = M + 6 if mapped else M
                rowmap = rng.permutation(rows_c)[:M] if mapped else np.arange(M)
                rA, rB = Region(ctx, *sa, count=nz, data=A), Region(ctx, K, N, count=nz, data=B)
                rC = Region(ctx, rows_c, N, count=nz, fill="sentinel")                      # cz larger than one member
                kw = dict(batch=nz, stride_a=rA.stride, stride_b=rB.stride, cz=rC.stride)
                if mapped:
                    kw["rowmap"] = rowmap
                rc, splits = probe(ctx, ZRED, tA, 0, 1.0, rA, rB, 0.0, rC, options(**kw))
                what = f"z {P.name} nz {nz} {M}x{N}x{K} tA={tA} mapped={mapped} splits={splits}"
                assert rc == 0, what
                seen.add(splits)
                got = rC.result(what)
                keep = np.ones(rows_c, dtype=bool); keep[rowmap] = False
                for z in range(nz):
                    assert np.array_equal(got[z][keep].view(np.uint64), rC.host[rC.idx][z][keep].view(np.uint64)), what
                    P.check(got[z][rowmap], 1.0, op(A[z], tA), B[z], 0.0, None, f"{what} member {z}")
    assert 1 in seen and any(s >= 9 for s in seen), seen                  # the reduce kernel's tail alone, and its 8-group


def test_gemm_partials_z_refusals(ctx):
    M, N, K = 17, 15, 8
    for nz, tA, tB in ((17, 0, 0), (2, 1, 1), (2, 0, 1)):
        sa = (K, M) if tA else (M, K); sb = (N, K) if tB else (K, N)
        rA = Region(ctx, *sa, count=nz, data=np.ones((nz,) + sa)); rB = Region(ctx, *sb, count=nz, data=np.ones((nz,) + sb))
        rC = Region(ctx, M, N, count=nz, fill="sentinel")
        rc, _ = probe(ctx, ZRED, tA, tB, 1.0, rA, rB, 0.0, rC, options(batch=nz, stride_a=rA.stride, stride_b=rB.stride, cz=rC.stride))
        assert rc == ERR_INVALID, (nz, tA, tB)
        rC.assert_untouched()


# ---- gemm_sym_update -------------------------------------------------------------------------------------------------------------------
def _check_sym(P, out, X0, A, B, what):
    assert np.array_equal(out.view(np.uint64), out.T.copy().view(np.uint64)), what + ": X != X' bit for bit"
    K = A.shape[1]
    if P is G.Exact:
        R = X0 + A @ B.T
        assert np.array_equal(out, 0.5 * (R + R.T)), what
    else:
        R = X0.astype(LD) + A.astype(LD) @ B.astype(LD).T
        ref = LD(0.5) * (R + R.T)
        b = (K + 3) * EPS * (np.abs(A) @ np.abs(B).T + np.abs(X0)) * (1.0 - 1e-11)      # the bound of X + A B' with K + 3 ...
        b = 0.5 * (b + b.T)                                                             # ... symmetrised
        err = np.abs(out.astype(LD) - ref)
        assert (err <= b).all(), f"{what}: worst err/bound {float(np.nanmax(err / np.maximum(b, 1e-300))):.3g}"


@PASS
@pytest.mark.parametrize("n", (1, 15, 16, 17, 33, 100))
def test_gemm_sym_update(ctx, P, n):
    for K in (1, 40, 200):
        rng = _seed(16, n, K)
        A, B, X0 = P.gen(rng, (n, K)), P.gen(rng, (n, K)), P.gen(rng, (n, n))          # X0 is not symmetric: both triangles are read
        rA, rB, rX = Region(ctx, n, K, data=A), Region(ctx, n, K, data=B, off=2), Region(ctx, n, n, data=X0, fill="sentinel")
        rc, splits = probe(ctx, SYM, 0, 0, 0.0, rA, rB, 0.0, rX)
        what = f"sym {P.name} n {n} K {K} splits {splits}"
        assert rc == 0 and (splits > 1) == (K == 200), what
        _check_sym(P, rX.result(what)[0], X0, A, B, what)


@PASS
def test_gemm_sym_update_device_count(ctx, P):
    n, per, nmax, base = 33, 2, 100, 3
    for cnt in (0, 37, 100, 120):
        ke = per * min(cnt, nmax)
        rng = _seed(17, cnt)
        A, B, X0 = P.gen(rng, (n, per * nmax)), P.gen(rng, (n, per * nmax)), P.gen(rng, (n, n))
        Ah, Bh = A.copy(), B.copy(); Ah[:, ke:] = np.nan; Bh[:, ke:] = np.nan
        rA, rB, rX = Region(ctx, *A.shape, data=Ah), Region(ctx, *B.shape, data=Bh), Region(ctx, n, n, data=X0, fill="sentinel")
        rc, splits = probe(ctx, SYM, 0, 0, 0.0, rA, rB, 0.0, rX, options(use_count=1, iters=base + cnt, base=base, nmax=nmax, per=per))
        what = f"sym count {cnt} {P.name}"
        assert rc == 0 and splits == 3, what
        _check_sym(P, rX.result(what)[0], X0, A[:, :ke], B[:, :ke], what)


def test_gemm_sym_update_with_no_columns_leaves_x_alone(ctx):
    n = 17
    X0 = G.Exact.gen(_seed(18), (n, n))
    assert not np.array_equal(X0, X0.T)
    rA, rB, rX = Region(ctx, n, 0), Region(ctx, n, 0), Region(ctx, n, n, data=X0, fill="sentinel")
    assert probe(ctx, SYM, 0, 0, 0.0, rA, rB, 0.0, rX)[0] == 0
    rX.assert_untouched()
