"""The GEMM calls of the dual replay (csrc/dense_sign.hip, SignLyap::replay_t / residual_t) through dre_gemm_probe, at the orders the dual tests
run: square M = N = K = n, no transposition with beta = 0 (P V, E^-1 R, F T) and B transposed with beta != 0 (the accumulating
V/(2c) + (c/2) (P V) P') and with beta = 0 (T E^-T, Y E').  tests/test_gpu_gemm_family.py covers the entry point at its tile and split edges;
n = 33, 70 and 371 are no multiples of the 64 x 64 tile and take different split-K counts.  Judged as there: bit for bit on integer operands
and within (K + 2) eps (|alpha| |A| |B| + |beta| |C|) against np.longdouble."""
import numpy as np
import pytest

import _gemm_probe as G
from _gemm_probe import GEMM, Region, op, probe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", G.PASSES, ids=lambda p: p.name)
@pytest.mark.parametrize("n", [33, 70, 371])
def test_square_products_of_the_dual_replay(ctx, P, n):
    for i, (tB, alpha, beta) in enumerate(((0, 1.0, 0.0), (1, 0.5, 0.5), (1, 1.0, 0.0), (1, -2.0, 1.0))):
        rng = np.random.default_rng([109, n, i])
        A, B, C0 = P.gen(rng, (n, n)), P.gen(rng, (n, n)), P.gen(rng, (n, n))
        rA, rB = Region(ctx, n, n, data=A, ld=n), Region(ctx, n, n, data=B, ld=n, off=3)              # ld = n as the solver's operands
        rC = Region(ctx, n, n, data=C0 if beta != 0.0 else np.full((n, n), np.nan), fill="sentinel", ld=n)
        rc, splits = probe(ctx, GEMM, 0, tB, alpha, rA, rB, beta, rC)
        what = f"gemm {P.name} n={n} tB={tB} alpha={alpha} beta={beta} splits={splits}"
        assert rc == 0, what
        P.check(rC.result(what)[0], alpha, A, op(B, tB), beta, C0, what)
