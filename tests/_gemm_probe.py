"""ctypes glue for dre_gemm_probe (include/dre_hip.h) and the references of tests/test_gpu_gemm_family.py.

Every operand is a `Region`: `count` members of rows x cols (leading dimension ld > rows, member stride larger than a member) that begin `off`
elements into a flat device buffer with spare room behind them.  What surrounds the members is NaN for inputs (a read outside a view poisons
the result) and a sentinel ramp for outputs (compared bit for bit after the call).

Two passes judge a result, neither with a measured tolerance:
  Exact    integer operands in [-4, 4], alpha, beta in {1, -2, 0.5}: every product and partial sum is an exactly representable multiple of a
           power of two far below 2^53, so the float64 NumPy result is THE result and the device must match it bit for bit.
  Rounded  standard-normal operands against np.longdouble, componentwise
               |out - ref| <= (K + 2) eps (|alpha| |op A| |op B| + |beta| |C|),   eps = 2^-52:
           any summation order of K products, with or without FMA, costs at most gamma_K; the split-K reduction adds at most K / 64 further
           additions, the alpha, beta epilogue three roundings, zero padding exact zeros: together below (2K + 4) u = (K + 2) eps.
           The bound itself is evaluated in float64 and scaled by (1 - 1e-11), which exceeds its own rounding error (K <= 6000), so that the
           bound applied is never wider than the one stated.
"""
import ctypes as C

import numpy as np

import dre_amd as D

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble has no 64-bit mantissa here: the rounded pass would compare double against double"
EPS = 2.0 ** -52

GEMM, THIN, STRIDED, BATCHED, ROWS, ZRED, SYM = range(7)
ERR_INVALID = -1

ViewC = D._lib.GemmViewC
ProductC = D._lib.GemmProductC
OptionsC = D._lib.GemmProbeOptionsC


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def sentinel(n):
    return 1.0e6 + 0.5 * np.arange(n, dtype=np.float64)


class Region:
    """`count` column-major members of rows x cols inside a flat device buffer.  `data`: (count, rows, cols) or (rows, cols) values, or None to
    leave the members filled like their surroundings (`fill`: "nan" or "sentinel")."""

    def __init__(self, ctx, rows, cols, count=1, data=None, fill="nan", ld=None, stride=None, off=7, tail=11):
        self.ctx, self.rows, self.cols, self.count = ctx, rows, cols, count
        self.ld = ld if ld is not None else rows + 5
        ext = (cols - 1) * self.ld + rows if rows > 0 and cols > 0 else 0
        self.stride = stride if stride is not None else ext + 13
        self.off = off
        n = off + (count - 1) * self.stride + ext + tail
        self.host = sentinel(n) if fill == "sentinel" else np.full(n, np.nan)
        b, i, j = np.meshgrid(np.arange(count), np.arange(rows), np.arange(cols), indexing="ij")
        self.idx = off + b * self.stride + i + j * self.ld          # (count, rows, cols) -> flat index
        if data is not None:
            self.host[self.idx] = np.asarray(data, dtype=np.float64).reshape(count, rows, cols)
        self.inside = np.zeros(n, dtype=bool)
        self.inside[self.idx] = True
        p = C.c_void_p()
        ctx.chk(ctx.lib.dre_dense_upload(ctx.ptr, n, 1, _pd(self.host), n, C.byref(p)))
        self.dev = p

    def view(self, member=0, rows=None, cols=None, off=None, ld=None):
        return ViewC(self.dev, self.off + member * self.stride if off is None else off, self.ld if ld is None else ld,
                     self.rows if rows is None else rows, self.cols if cols is None else cols)

    def download(self):
        out = np.empty_like(self.host)
        self.ctx.chk(self.ctx.lib.dre_dense_download(self.ctx.ptr, self.dev, _pd(out), out.size))
        return out

    def result(self, what=""):
        """The members after the call, (count, rows, cols); everything around them must be bit-identical to what was uploaded."""
        got = self.download()
        assert np.array_equal(got.view(np.uint64)[~self.inside], self.host.view(np.uint64)[~self.inside]), f"{what}: wrote outside the view"
        return got[self.idx]

    def assert_untouched(self, what=""):
        assert np.array_equal(self.download().view(np.uint64), self.host.view(np.uint64)), f"{what}: the buffer was written"

    def free(self):
        if self.dev is not None:
            self.ctx.lib.dre_dense_free(self.ctx.ptr, self.dev)
            self.dev = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def options(**kw):
    """dre_gemm_probe_options from keywords; lists become C arrays that the returned object keeps alive."""
    o = OptionsC()
    keep = []
    for k, v in kw.items():
        if k in ("member_on", "rowmap"):
            arr = (C.c_int32 * max(len(v), 1))(*[int(x) for x in v])
            keep.append(arr); setattr(o, k, C.cast(arr, C.POINTER(C.c_int32)))
        elif k == "coef":
            arr = (C.c_double * len(v))(*[float(x) for x in v])
            keep.append(arr); o.coef = C.cast(arr, C.POINTER(C.c_double))
        elif k == "prod":
            arr = (ProductC * max(len(v), 1))(*v)
            keep.append(arr); o.prod = C.cast(arr, C.POINTER(ProductC)); o.nprod = len(v)
        elif k == "tile_sumsq":
            o.tile_sumsq = v
        else:
            setattr(o, k, int(v))
    o._keep = keep
    return o


def _as_view(x):
    if x is None:
        return None
    return C.byref(x if isinstance(x, ViewC) else x.view())


def probe(ctx, kind, tA, tB, alpha, A, B, beta, Cv, opts=None):
    """One call; A, B, Cv are Regions (member 0 is the view), ViewC's or None.  Returns (status, splits)."""
    s = C.c_int(-1)
    rc = ctx.lib.dre_gemm_probe(ctx.ptr, kind, int(tA), int(tB), float(alpha), _as_view(A), _as_view(B), float(beta), _as_view(Cv),
                                C.byref(opts) if opts is not None else None, C.byref(s))
    return rc, s.value


def op(X, t):
    return X.T if t else X


class Exact:
    name = "exact"

    @staticmethod
    def gen(rng, shape):
        return rng.integers(-4, 5, size=shape).astype(np.float64)

    @staticmethod
    def check(out, alpha, Aop, Bop, beta, C0, what=""):
        ref = alpha * (Aop @ Bop)
        if beta != 0.0:
            ref = ref + beta * C0
        assert np.array_equal(out, ref), f"{what}: {np.count_nonzero(out != ref)} of {ref.size} entries differ from the exact result"


class Rounded:
    name = "rounded"

    @staticmethod
    def gen(rng, shape):
        return rng.standard_normal(shape)

    @staticmethod
    def ref_and_bound(alpha, Aop, Bop, beta, C0, extra=2):
        K = Aop.shape[1]
        ref = LD(alpha) * (Aop.astype(LD) @ Bop.astype(LD))
        mag = abs(alpha) * (np.abs(Aop) @ np.abs(Bop))
        if beta != 0.0:
            ref = ref + LD(beta) * C0.astype(LD)
            mag = mag + abs(beta) * np.abs(C0)
        return ref, (K + extra) * EPS * mag * (1.0 - 1e-11)

    @staticmethod
    def check(out, alpha, Aop, Bop, beta, C0, what=""):
        ref, bound = Rounded.ref_and_bound(alpha, Aop, Bop, beta, C0)
        err = np.abs(out.astype(LD) - ref)
        ok = err <= bound                      # (a NaN in out fails here)
        assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} entries beyond the bound, worst err/bound {float(np.nanmax(err / np.maximum(bound, 1e-300))):.3g}"


PASSES = (Exact, Rounded)
