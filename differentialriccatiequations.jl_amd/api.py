"""Host-side mirror of the reference's CommonSolve surface for the low-rank GDRE path.

Same names, argument meaning and error behaviour as mpimd-csc/DifferentialRiccatiEquations.jl v0.5.5
(`GDREProblem`, `GALEProblem`, `Ros1`, `Ros2`, `ADI`, `Shifts.{Cyclic,Projection,Heuristic,Wrapped}`, `lowrank`,
`concatenate_`, `compress_`, `residual`, `solve`, `Callbacks`), written in Python because the reference's own
host language (Julia) is not installed in this image; the Julia shim with identical structure is
`julia/DREHip.jl`.  Every arithmetic operation is executed by libdre_hip on the GPU through the C ABI —
this module holds no numerical fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import time
import warnings
import weakref
import dataclasses
from dataclasses import dataclass, field
from typing import Any, Optional

import numpy as np
import scipy.sparse as sp

from . import device as dev
from ._lib import DREError

EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------
# LDLᵀ                                                          /root/reference/src/LDLt.jl
# ------------------------------------------------------------------------------------------------
class LDLt:
    """Lazy `sum_i alpha_i L_i D_i L_i'` (LDLt.jl:29-33).  Factors live on the host as NumPy arrays or,
    for results produced by the engine, on the device until first touched."""

    def __init__(self, alphas, Ls, Ds, _handle: dev.DeviceLDLt | None = None):
        self._alphas, self._Ls, self._Ds = list(alphas), list(Ls), list(Ds)
        self._handle = _handle

    # lazy materialisation of device results
    def _host(self):
        if self._handle is not None and not self._Ls:
            self._handle.canonicalize()     # engine results carry a tridiagonal D; users get the reference form
            a, L, D = self._handle.destructure()
            self._alphas, self._Ls, self._Ds = [a], [L], [D]
        return self

    def _factors_any_form(self):
        """(alpha, L, D) of a single-block view in WHATEVER form the engine holds (D may be a band matrix): enough for products
        such as B'LD or E'L; skips the eigen-decomposition that the reference form (`alpha, L, D = X`) costs."""
        if self._handle is not None and not self._Ls:
            if getattr(self, "_raw", None) is None:
                self._raw = self._handle.destructure()
            return self._raw
        return tuple(self)

    @property
    def alphas(self):
        return self._host()._alphas

    @property
    def Ls(self):
        return self._host()._Ls

    @property
    def Ds(self):
        return self._host()._Ds

    @property
    def n(self):
        if self._handle is not None and not self._Ls:
            return self._handle.info()[0]
        return self._Ls[0].shape[0]

    def size(self):
        return (self.n, self.n)

    def rank(self):                      # LDLt.jl:112
        if self._handle is not None and not self._Ls:
            return self._handle.info()[1]
        return sum(L.shape[1] for L in self._Ls)

    def iszero(self):                    # LDLt.jl:114
        if self._handle is not None and not self._Ls:
            return self.rank() == 0      # engine results: no download / canonicalisation just to look at alpha
        return self.rank() == 0 or all(a == 0 for a in self.alphas)

    def zero(self):                      # LDLt.jl:116-121
        return lowrank(np.zeros((self.n, 0)), np.zeros((0, 0)))

    def dense(self):                     # Matrix(X), LDLt.jl:41-51 (testing only)
        M = np.zeros((self.n, self.n))
        for a, L, D in zip(self.alphas, self.Ls, self.Ds):
            M += L @ (a * D) @ L.T
        return M

    def __add__(self, other):            # LDLt.jl:131-148
        if self.n != other.n:
            raise ValueError(f"outer dimensions must match, got {self.n} and {other.n} instead")
        if self.iszero():
            return other
        if other.iszero():
            return self
        return LDLt(self.alphas + other.alphas, self.Ls + other.Ls, self.Ds + other.Ds)

    def __neg__(self):                   # LDLt.jl:150-153
        return LDLt([-a for a in self.alphas], self.Ls, self.Ds)

    def __sub__(self, other):
        return self + (-other)

    def __rmul__(self, alpha):           # LDLt.jl:156-159: factors are shared, only alphas change
        out = LDLt([alpha * a for a in self.alphas], [], [])
        out._Ls, out._Ds = self.Ls, self.Ds
        return out

    def __truediv__(self, alpha):
        return (1.0 / alpha) * self

    def __eq__(self, other):             # LDLt.jl:35
        return (self.alphas == other.alphas and len(self.Ls) == len(other.Ls)
                and all(np.array_equal(a, b) for a, b in zip(self.Ls, other.Ls))
                and all(np.array_equal(a, b) for a, b in zip(self.Ds, other.Ds)))

    def __iter__(self):                  # alpha, L, D = X  (LDLt.jl:54-60)
        if len(self.Ls) > 1:
            compress_(self)
        return iter((self.alphas[0], self.Ls[0], self.Ds[0]))

    # upload as a device object (one device block per host block)
    def _to_device(self, ctx, pencil) -> dev.DeviceLDLt:
        if self._handle is not None and self._handle.pencil is pencil and not self._dirty_host():
            return self._handle
        if self.rank() == 0:
            return dev.DeviceLDLt.zero(ctx, pencil, self.n)
        h = None
        for a, L, D in zip(self.alphas, self.Ls, self.Ds):
            D = np.eye(L.shape[1]) if D is None else np.asarray(D, dtype=float)
            b = dev.DeviceLDLt.create(ctx, pencil, L, D, a)
            h = b if h is None else h.add(b)
        return h

    def _dirty_host(self):
        return False

    def _adopt(self, handle: dev.DeviceLDLt):
        a, L, D = handle.destructure()
        self._alphas[:] = [a]
        self._Ls[:] = [L]
        self._Ds[:] = [D]


def lowrank(L, D=None) -> LDLt:
    """lowrank(L, D=I)  (LDLt.jl:24-27)"""
    L = np.asfortranarray(np.asarray(L, dtype=float))
    D = np.eye(L.shape[1]) if D is None else np.asarray(D, dtype=float)
    return LDLt([1.0], [L], [D])


def _on_device(X: LDLt, ctx=None):
    ctx = ctx or dev.default_context()
    return X._to_device(ctx, None)


def concatenate_(X: LDLt) -> LDLt:
    """concatenate!(X)  (LDLt.jl:174-191)"""
    if len(X.alphas) == 1:
        return X
    h = _on_device(X)
    h.concatenate()
    X._adopt(h)
    return X


def compress_(X: LDLt) -> LDLt:
    """compress!(X)  (LDLt.jl:204-225) — QR + early-terminating symmetric eigensolver on the GPU."""
    if X.rank() == 0:
        return X
    h = _on_device(X)
    h.compress()
    X._adopt(h)
    return X


def norm(X: LDLt) -> float:
    """norm(X::LDLᵀ)  (LDLt.jl:77-89)"""
    if X.rank() == 0:
        return 0.0
    return _on_device(X).norm()


def orthf(L):
    """orthf(L) -> Q, R  (LDLt.jl:237-245)"""
    ctx = dev.default_context()
    Ld = ctx.upload(L)
    q, r = C.c_void_p(), C.c_void_p()
    ctx.chk(ctx.lib.dre_orthf(ctx.ptr, Ld.ptr, C.byref(q), C.byref(r)))
    return dev.DenseMatrix(ctx, q).numpy(), dev.DenseMatrix(ctx, r).numpy()


def sym_eigh(A, method="jacobi", tol=None, ctx=None, return_stats=False):
    """eigh(A) of a dense symmetric matrix on the device: (w, V) with w ascending and A V = V diag(w).
    method "jacobi": the whole-device block Jacobi solver (dre_sym_eig_jacobi; converged when off(A) <= tol ||A||_F, tol None: n eps);
    method "ql": the library's Householder + implicit-QL solver (dre_sym_eig), which returns the eigenpairs its early-terminating reduction
    kept (all of them unless A is numerically rank deficient) and ignores tol; it is that solver whatever the context option sym_eig_method
    says (the option chooses the solver of the compressions, not of this call).  return_stats adds dict(sweeps, rounds) (zeros for "ql").
    A non-square A, an A that is not symmetric to 100 eps max|A|, and an unknown method are errors before anything runs on the device."""
    A = np.asarray(A, dtype=float)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"sym_eigh: a square matrix is expected, got shape {A.shape}; nothing was run on the device")
    if method not in ("jacobi", "ql"):
        raise ValueError(f"sym_eigh: unknown method {method!r} (\"jacobi\" or \"ql\"); nothing was run on the device")
    if tol is not None and not float(tol) > 0.0:
        raise ValueError("sym_eigh: tol must be positive; nothing was run on the device")
    if A.size and np.isfinite(A).all():           # (a non-finite entry is the device solver's DRE_ERR_INVALID)
        asym = np.abs(A - A.T).max()
        if asym > 100 * np.finfo(float).eps * np.abs(A).max():
            raise ValueError(f"sym_eigh: the matrix is not symmetric (max |A - A'| = {asym:.3e}); nothing was run on the device")
    n = A.shape[0]
    stats = dict(sweeps=0, rounds=0)
    if n == 0:
        w, V = np.zeros(0), np.zeros((0, 0))
        return (w, V, stats) if return_stats else (w, V)
    ctx = ctx or dev.default_context()
    Ad = ctx.upload(np.asfortranarray(A))
    wp, vp = C.c_void_p(), C.c_void_p()
    if method == "jacobi":
        ii = (C.c_int64 * 2)()
        ctx.chk(ctx.lib.dre_sym_eig_jacobi(ctx.ptr, Ad.ptr, float(tol) if tol is not None else 0.0, C.byref(wp), C.byref(vp), ii))
        stats = dict(sweeps=int(ii[0]), rounds=int(ii[1]))
    else:
        ctx.chk(ctx.lib.dre_sym_eig(ctx.ptr, Ad.ptr, 4.0, C.byref(wp), C.byref(vp)))
    w, V = dev.DenseMatrix(ctx, wp).numpy().ravel(), dev.DenseMatrix(ctx, vp).numpy()
    return (w, V, stats) if return_stats else (w, V)


def delta(a, b):
    """Stuff.delta (src/Stuff.jl:21)"""
    return np.linalg.norm(a - b) / max(np.linalg.norm(a), np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------
# LowRankUpdate                                              /root/reference/src/LowRankUpdate.jl
# ------------------------------------------------------------------------------------------------
@dataclass
class LowRankUpdate:
    """Lazy `A + inv(alpha)*U*V` with sparse `A` (LowRankUpdate.jl:18-26)."""
    A: Any
    alpha: float
    U: np.ndarray
    V: np.ndarray

    @property
    def shape(self):
        return self.A.shape


def lr_update(A, alpha, U, V):
    """lr_update (LowRankUpdate.jl:38-39): dense -> Matrix, sparse -> lazy."""
    if sp.issparse(A) or isinstance(A, ScaledPencil):
        return LowRankUpdate(A, alpha, np.asarray(U, float), np.asarray(V, float))
    return np.asarray(A) + (1.0 / alpha) * (np.asarray(U) @ np.asarray(V))


# ------------------------------------------------------------------------------------------------
# Shifts                                                      /root/reference/src/Shifts.jl, src/shifts/*
# ------------------------------------------------------------------------------------------------
def _hash_key(x):
    """Structural key of an option value: shift lists (list / tuple / ndarray) by their entries, everything else by itself."""
    if isinstance(x, np.ndarray):
        return ("values",) + tuple(x.ravel().tolist())
    if isinstance(x, (list, tuple)):
        return ("values",) + tuple(_hash_key(v) if isinstance(v, (list, tuple, np.ndarray)) else v for v in x)
    return x


class Shifts:
    class Strategy:
        """Strategies hash and compare by STRUCTURE: two separately built `Cyclic([1.0])` — or `ADI(shifts=...)` options holding them — give the
        same hash within a session (test/hash.jl; the reference defines `Base.hash` for `Cyclic` and `Wrapped`, shifts/helpers.jl:23-27,53-58,
        `Projection` and `Heuristic` are immutable structs and hash by their fields)."""
        _tag = 0

        def _key(self):
            return ()

        # User-defined strategies (the reference's extension point Shifts.init / update! / take!, src/Shifts.jl:79-116; batch form take_many!,
        # shifts/helpers.jl:60-89; example: the Dummy strategy of test/Shifts.jl:133-163): subclass Strategy and define
        #     take_many(self, hist) -> iterable of shifts     hist: n x w array, what update! handed over (the residual factor R at the start of a
        #                                                     solve, then the last `n_history` increments V, oldest first)
        #     init(self, prob)                                 optional, called at the start of every Lyapunov solve with (E, A) of the equation
        #     n_history                                        optional attribute (default 2)
        # Shifts need a negative real part; a complex shift is followed by its conjugate (adi.jl:190).  `Wrapped(f, strategy)` applies f to
        # every batch (shifts/helpers.jl:95-120).

        def __hash__(self):
            return hash((type(self)._tag,) + tuple(_hash_key(v) for v in self._key()))

        def __eq__(self, other):
            return type(other) is type(self) and tuple(_hash_key(v) for v in self._key()) == tuple(_hash_key(v) for v in other._key())

        def __repr__(self):
            return f"{type(self).__name__}({', '.join(getattr(v, '__name__', None) or repr(v) for v in self._key())})"

    class Cyclic(Strategy):
        """Cyclic(values) or Cyclic(strategy)  (shifts/helpers.jl:19-21,91-93)"""
        _tag = 21                                   # shifts/helpers.jl:24

        def __init__(self, inner):
            self.inner = inner

        def _key(self):
            return (self.inner,)

    class Wrapped(Strategy):
        """Wrapped(func, strategy)  (shifts/helpers.jl:48-51)"""
        _tag = 22                                   # shifts/helpers.jl:54

        def __init__(self, func, inner):
            self.func, self.inner = func, inner

        def _key(self):
            return (self.func, self.inner)

    class Projection(Strategy):
        """Projection(u)  (shifts/projection.jl:25-33)"""

        def __init__(self, u: int):
            if u % 2 == 1:
                raise ValueError(f"History must be even; got {u}")
            self.n_history = u

        _tag = 23

        def _key(self):
            return (self.n_history,)

    class Heuristic(Strategy):
        """Heuristic(nshifts, k₊, k₋)  (shifts/heuristic.jl:22-31)"""
        _tag = 24

        def __init__(self, nshifts, k_plus, k_minus):
            self.nshifts, self.k_plus, self.k_minus = nshifts, k_plus, k_minus

        def _key(self):
            return (self.nshifts, self.k_plus, self.k_minus)

    # helpers (shifts/helpers.jl:122-140)
    @staticmethod
    def isstable(v):
        return np.real(v) < 0

    @staticmethod
    def flip(x):
        if isinstance(x, complex):
            return complex(-x.real, x.imag)
        return -x

    @staticmethod
    def stabilize_ritz_values(lam, desc):
        assert len(lam) > 0
        nun = sum(1 for v in lam if not Shifts.isstable(v))
        if 0 < nun < len(lam):
            warnings.warn(f"Discarding unstable Ritz values of {desc}")
            return [v for v in lam if Shifts.isstable(v)]
        if nun == len(lam):
            warnings.warn(f"All Ritz values of {desc} are unstable; flipping along imaginary axis")
            return [Shifts.flip(v) for v in lam]
        return list(lam)

    @staticmethod
    def safe_sort(shifts):
        return sorted(shifts, key=lambda v: (np.real(v), abs(np.imag(v))))

    @staticmethod
    def heuristic(R, nshifts=None):
        """Penzl's greedy selection (shifts/heuristic.jl:82-101)."""
        R = [complex(v) for v in R]
        nshifts = len(R) if nshifts is None else nshifts

        def s(t, P):
            out = 1.0
            for p in P:
                out *= abs(t - p) / abs(t + p)
            return out

        p = min(R, key=lambda p: max(s(t, (p,)) for t in R))
        P = [p] if p.imag == 0 else [p, p.conjugate()]
        while len(P) < nshifts:
            p = max(R, key=lambda t: s(t, P))
            P += [p] if p.imag == 0 else [p, p.conjugate()]
        return P


def _arnoldi_ritz(op, b0, k, desc):
    """compute_ritz_values (shifts/heuristic.jl:103-130); `op` runs on the device."""
    n = b0.shape[0]
    H = np.zeros((k + 1, k))
    V = np.zeros((n, k + 1))
    V[:, 0] = b0 / np.linalg.norm(b0)
    for j in range(k):
        w = np.array(op(V[:, j]), dtype=float).reshape(-1)
        for _ in range(2):
            for i in range(j + 1):
                g = V[:, i] @ w
                H[i, j] += g
                w -= V[:, i] * g
        beta = np.linalg.norm(w)
        H[j + 1, j] = beta
        V[:, j + 1] = w / beta
    return Shifts.stabilize_ritz_values(list(np.linalg.eigvals(H[:k, :k])), desc)


def heuristic_shifts(strategy: "Shifts.Heuristic", pencil: dev.Pencil, lr=None, on_device=True):
    """Shifts.init(::Heuristic, prob) (shifts/heuristic.jl:39-66).  The two Arnoldi runs (Ritz values of E^-1 F and F^-1 E from
    ones(n)) execute on the device in one call (`dre_heuristic_ritz`); `lr = (alpha, U, V)` is the low-rank part of
    F = A + inv(alpha) U V (LowRankUpdate): products add it, solves go through Sherman-Morrison-Woodbury exactly like the reference's
    inner solvers (heuristic.jl:51-60).  Stabilisation and the greedy min-max selection are host logic (Shifts.heuristic).
    `on_device=False` runs the Arnoldi recurrences in NumPy with device solves/SpMMs (kept as a cross-check)."""
    if not on_device:
        return _heuristic_shifts_host_arnoldi(strategy, pencil, lr)
    ctx = pencil.ctx
    kp, km = int(strategy.k_plus), int(strategy.k_minus)
    pr, pi_, mr, mi = np.zeros(kp), np.zeros(kp), np.zeros(km), np.zeros(km)
    U = Vt = None
    alpha = 1.0
    if lr is not None:
        alpha, Uh, Vh = lr
        U, Vt = ctx.upload(np.asarray(Uh, dtype=float)), ctx.upload(np.ascontiguousarray(np.asarray(Vh, dtype=float).T))
    as_pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ctx.chk(ctx.lib.dre_heuristic_ritz(ctx.ptr, pencil.ptr, 1.0, 0.0, float(alpha), U.ptr if U else None, Vt.ptr if Vt else None,
                                       kp, km, as_pd(pr), as_pd(pi_), as_pd(mr), as_pd(mi)))
    Rp = Shifts.stabilize_ritz_values(list(pr + 1j * pi_), "E⁻¹A")
    Rm = Shifts.stabilize_ritz_values(list(mr + 1j * mi), "A⁻¹E")
    return Shifts.heuristic(list(Rp) + [1.0 / v for v in Rm], strategy.nshifts)


def _heuristic_shifts_host_arnoldi(strategy, pencil, lr=None):
    n = pencil.n
    b0 = np.ones(n)
    fE = pencil.factor(0.0, 1.0)
    fA = pencil.factor(1.0, 0.0)
    if lr is None:
        mulF = lambda x: pencil.spmm(1, x.reshape(-1, 1)).numpy()
        solveF = lambda y: fA.solve(y)
    else:
        alpha, U, V = lr
        U, Vt = np.asarray(U, dtype=float), np.asarray(V, dtype=float).T
        W = np.asarray(fA.solve(Vt))                                  # A0'^-1 V'   (n x m)
        Sm = alpha * np.eye(U.shape[1]) + U.T @ W
        mulF = lambda x: pencil.spmm(1, x.reshape(-1, 1)).numpy() + (Vt @ (U.T @ x.reshape(-1, 1))) / alpha

        def solveF(y):
            z = np.asarray(fA.solve(y)).reshape(n, -1)
            return z - W @ np.linalg.solve(Sm, U.T @ z)
    Rp = _arnoldi_ritz(lambda x: fE.solve(mulF(x)), b0, strategy.k_plus, "E⁻¹A")
    Rm = _arnoldi_ritz(lambda x: solveF(pencil.spmm(0, x.reshape(-1, 1)).numpy()), b0, strategy.k_minus, "A⁻¹E")
    return Shifts.heuristic(list(Rp) + [1.0 / v for v in Rm], strategy.nshifts)


def _user_strategy(strategy):
    """(strategy object with take_many, post-processing functions) of a user-defined strategy, possibly inside Wrapped layers; None otherwise."""
    funcs = []
    s = strategy
    while isinstance(s, Shifts.Wrapped):
        funcs.append(s.func)
        s = s.inner
    if isinstance(s, Shifts.Strategy) and callable(getattr(s, "take_many", None)):
        return s, funcs[::-1]                   # innermost wrapper first (shifts/helpers.jl:113-120)
    return None


def _shift_callback(strategy, prob_info):
    """ctypes trampoline for a user-defined strategy (dre_shift_fn).  Returns (function pointer, keep-alive, errors)."""
    from ._lib import SHIFT_FN
    s, funcs = _user_strategy(strategy)
    errors = []

    def tramp(user, restart, n, hist_cols, hist_p, ldh, capacity, re_p, im_p, count_p):
        try:
            if restart and callable(getattr(s, "init", None)):
                s.init(prob_info)
            H = np.empty((ldh, hist_cols), order="F")
            if hist_cols > 0:
                _hip_memcpy(H.ctypes.data, hist_p, H.nbytes, 2)               # device -> host
            vals = list(s.take_many(H[:n, :]))
            for f in funcs:
                vals = list(f(vals))
            if not 1 <= len(vals) <= capacity:
                raise ValueError(f"take_many returned {len(vals)} shifts (1 .. {capacity} expected)")
            for i, v in enumerate(vals):
                v = complex(v)
                re_p[i], im_p[i] = v.real, v.imag
            count_p[0] = len(vals)
            return 0
        except Exception as e:                                                # no exception may cross the C boundary
            errors.append(e)
            return 1

    cb = SHIFT_FN(tramp)
    return cb, (cb, errors)


def _resolve_shifts(strategy, pencil, lr=None):
    """Map a strategy object to (shift_kind, n_history, values) of the C ABI."""
    S = Shifts
    if isinstance(strategy, S.Projection):
        return 1, strategy.n_history, None
    if _user_strategy(strategy) is not None:
        return 3, int(getattr(_user_strategy(strategy)[0], "n_history", 2)), None
    if isinstance(strategy, S.Cyclic):
        inner = strategy.inner
        if isinstance(inner, S.Heuristic):
            return 2, 2, (inner.nshifts, inner.k_plus, inner.k_minus)       # resolved inside the engine, per Lyapunov solve (adi.jl:54)
        elif isinstance(inner, S.Wrapped):
            if not isinstance(inner.inner, S.Heuristic):
                raise NotImplementedError("Cyclic(Wrapped(f, s)) is supported for s = Heuristic only")
            vals = list(inner.func(heuristic_shifts(inner.inner, pencil, lr)))
        elif isinstance(inner, S.Strategy):
            raise NotImplementedError(f"Cyclic({type(inner).__name__}) is not supported")
        else:
            vals = list(inner)
        if len(vals) == 0:
            raise ValueError("Cyclic: empty shift list")
        return 0, 2, vals
    if isinstance(strategy, S.Heuristic):
        raise NotImplementedError("use Cyclic(Heuristic(...)) — a bare Heuristic list would be exhausted")
    raise TypeError(f"unknown shift strategy {strategy!r}")


# ------------------------------------------------------------------------------------------------
# Problems, algorithms                    src/lyapunov/types.jl, src/riccati/types.jl, DifferentialRiccatiEquations.jl:55-60
# ------------------------------------------------------------------------------------------------
@dataclass
class GALEProblem:
    """A'XE + E'XA = -C with low-rank C (lyapunov/types.jl:10-16)."""
    E: Any
    A: Any
    C: LDLt


# ------------------------------------------------------------------------------------------------
# Block linear solvers                       src/blocklinear/types.jl:10-62, backslash.jl, sherman-morrison-woodbury.jl
# ------------------------------------------------------------------------------------------------
@dataclass
class BlockLinearProblem:
    """A X = B with a block right-hand side (blocklinear/types.jl:10-13)."""
    A: Any
    B: np.ndarray


class BlockLinearSolver:
    """Plug-in point of the reference (blocklinear/types.jl:15-30): subclass and implement `solve(prob) -> X` (the fallback protocol of
    types.jl:46-60).  Inside ADI the engine hands over the SPARSE shifted system  (cA A' + (cE_re + i cE_im) E') X = B  as a SciPy
    matrix + a host array — the role of ALG in `ShermanMorrisonWoodbury(ALG, alg)`; the rank-m correction stays on the device.
    A subclass that wants to stay on the device overrides `solve_device(n, nrhs, cA, cE_re, cE_im, B_ptr, Xre_ptr, Xim_ptr) -> int`
    (raw device pointers, exactly `dre_block_solver_fn` of include/dre_hip.h)."""

    def solve(self, prob: BlockLinearProblem):
        raise NotImplementedError

    solve_device = None


class Backslash(BlockLinearSolver):
    """`Backslash()` (blocklinear/backslash.jl): the library's own sparse direct solver (multifrontal LU on the device)."""

    def solve(self, prob: BlockLinearProblem):
        # `Backslash()` is a TAG in this package: the engine recognises it and runs its own multifrontal LU on the device (csrc/sparse.hip);
        # there is no host implementation behind it and no CPU fallback — a subclass that wants a host solve must bring its own `solve`
        raise DREError("Backslash() selects the library's device solver; it has no host-side solve().  Subclass BlockLinearSolver and "
                       "implement solve() (or solve_device) for a custom inner solver (blocklinear/types.jl:46-60)")


@dataclass
class ShermanMorrisonWoodbury(BlockLinearSolver):
    """`ShermanMorrisonWoodbury(alg_sparse, alg_dense)` (blocklinear/types.jl:35-39): `alg_sparse` solves with the sparse part,
    the small dense capacitance system is always solved on the device."""
    alg_sparse: Any = field(default_factory=Backslash)
    alg_dense: Any = field(default_factory=Backslash)


_hip_rt = None


def _hip_memcpy(dst, src, nbytes, kind):
    global _hip_rt
    if _hip_rt is None:
        _hip_rt = C.CDLL("libamdhip64.so")
        _hip_rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip_rt.hipMemcpy.restype = C.c_int
    rc = _hip_rt.hipMemcpy(dst, src, nbytes, kind)
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed with {rc}")


def _inner_solver_callback(inner_alg, E, A0):
    """ctypes trampoline for a user BlockLinearSolver (dre_block_solver_fn).  Returns (function pointer, keep-alive) or (None, None)."""
    from ._lib import BLOCK_SOLVER_FN
    if inner_alg is None or type(inner_alg) is Backslash:
        return None, None
    alg = inner_alg.alg_sparse if isinstance(inner_alg, ShermanMorrisonWoodbury) else inner_alg
    if alg is None or type(alg) is Backslash:
        return None, None
    if isinstance(A0, ScaledPencil):          # the library hands the trampoline the combined coefficients of the base pencil (E, A)
        A0 = A0.A
    Et, At = sp.csc_matrix(E).T.tocsc(), sp.csc_matrix(A0).T.tocsc()
    errors = []

    def tramp(user, n, nrhs, cA, cE_re, cE_im, Bp, Xrp, Xip):
        try:
            if alg.solve_device is not None:
                return int(alg.solve_device(n, nrhs, cA, cE_re, cE_im, Bp, Xrp, Xip))
            B = np.empty((n, nrhs), order="F")
            _hip_memcpy(B.ctypes.data, Bp, B.nbytes, 2)                       # device -> host
            cE = complex(cE_re, cE_im) if cE_im != 0.0 else cE_re
            X = np.asarray(alg.solve(BlockLinearProblem((cA * At + cE * Et).tocsc(), B)))
            Xr = np.asfortranarray(X.real.astype(np.float64))
            _hip_memcpy(Xrp, Xr.ctypes.data, Xr.nbytes, 1)                    # host -> device
            if Xip:
                Xi = np.asfortranarray(np.imag(X).astype(np.float64))
                _hip_memcpy(Xip, Xi.ctypes.data, Xi.nbytes, 1)
            return 0
        except Exception as e:                                                # no exception may cross the C boundary
            errors.append(e)
            return 1

    cb = BLOCK_SOLVER_FN(tramp)
    return cb, (cb, errors)


@dataclass
class ADI:
    """ADI options (lyapunov/types.jl:20-30)."""
    maxiters: int = 100
    reltol: Optional[float] = None
    abstol: Optional[float] = None
    shifts: Any = field(default_factory=lambda: Shifts.Projection(2))
    ignore_initial_guess: bool = False
    compression_interval: int = 10
    compression: bool = True
    warn_convergence: bool = True
    inner_alg: Any = None             # None / Backslash(): the device multifrontal LU; a BlockLinearSolver (or SMW(solver, ...)) plugs in
    # engine knob (not in the reference): True = eigen-based truncation at every compression, exactly the
    # reference's arithmetic; False = Krylov-truncated compression (same accuracy class, far cheaper on a GPU)
    compress_exact: bool = False

    def __hash__(self):
        """Structural hash over every property, order independent (lyapunov/types.jl:34-40: `hv ⊻= hash(p, hash(getproperty(alg, p)))`, seed 42) —
        a dataclass with `eq` would otherwise be unhashable, and DrWatson-style bookkeeping keys on `hash(ADI(...))` (test/hash.jl)."""
        hv = hash(42)
        for f in dataclasses.fields(self):
            hv ^= hash((f.name, hash(_hash_key(getattr(self, f.name)))))
        return hv


@dataclass
class GDREProblem:
    """E'ẊE = C'C + A'XE + E'XA − E'XBB'XE, X(t0) = X0 (riccati/types.jl:11-20)."""
    E: Any
    A: Any
    B: np.ndarray
    C: np.ndarray
    X0: Any
    tspan: tuple


@dataclass
class DRESolution:
    """riccati/types.jl:35-39"""
    X: list
    K: list
    t: np.ndarray


@dataclass
class Ros1:
    inner_alg: Optional[ADI] = None


@dataclass
class Ros2:
    inner_alg: Optional[ADI] = None


@dataclass
class MatrixSign:
    """Dense GALE and GARE algorithm tag (in the place of the reference's `BartelsStewart`, lyapunov/bartels-stewart.jl): the generalized
    matrix-sign-function iteration on the device.  It requires a c-stable pencil; otherwise DREError(-7, DRE_ERR_NOT_STABLE).
    Any n up to 46340 (the device's index limit) whose (maxiters + 26) n^2 doubles fit in device memory: the inversions use the register
    pivoting panel for n <= 4096 and the tournament panel above (context option dense_gj_panel).
    tol None: 10 n eps (stop when ||Z + E||_F <= tol ||E||_F); max_refine: refinement steps by replay while the relative residual
    exceeds 100 n eps.
    For a GAREProblem (solve_gare_dense): the sign iteration of the 2n x 2n Hamiltonian pencil (n <= 23170; tol None: 10 (2n) eps on the
    relative step) and max_refine Newton-Kleinman steps."""
    maxiters: int = 50
    tol: Optional[float] = None
    max_refine: int = 2


@dataclass(frozen=True)
class StepControl:
    """Step-size control of the dense Ros2 path: `solve(prob, Ros2(MatrixSign()), dt=dt0, adaptive=StepControl(...))`.  A trial step of size τ is
    judged by Ros2's embedded first-order solution: D = Xnew − (X + τ K1), err = sqrt(mean_ij (D_ij / (atol + rtol·max(|X_ij|, |Xnew_ij|)))²);
    it is accepted iff err ≤ 1 and the next size is τ·clamp(0.9·err^(−1/2), 0.2, 5) (no growth right after a rejection), kept inside
    [dt_min, dt_max].  `tspan[1]` and the `tstops` (strictly between the ends of tspan, strictly monotone in the direction of integration) are hit
    exactly.  A rejection at dt_min, or more than max_steps trial steps (rejected ones included), raises DREError(-8, DRE_ERR_STEP)."""
    rtol: float = 1e-3
    atol: float = 1e-6
    dt_min: float = 0.0
    dt_max: float = math.inf
    max_steps: int = 10_000
    tstops: tuple = ()


@dataclass(frozen=True)
class FactoredSign:
    """Low-rank GALE algorithm tag: the matrix-sign-function iteration on the densified pencil with the kept (P_k, c_k) sequence applied to the
    *factor* of the right-hand side (Benner & Quintana-Ortí 1999 §4).  LDLᵀ in, LDLᵀ out, no shifts; needs a c-stable pencil like `MatrixSign`
    (DREError(-7) otherwise) and (maxiters + 7) n² doubles of device memory.  Distinct from `MatrixSign` on purpose: that tag keeps selecting the
    dense solvers.
    tol None: 10 n eps for the sign iteration; rtol None: n eps, the truncation threshold of `compress!` (LDLt.jl:237-245), relative to the
    largest |eigenvalue|; max_width: the factor is compressed whenever it grows wider (and once at the end); max_refine: corrections by
    replaying the compressed residual factor while the relative residual exceeds 100 n eps + 10 rtol."""
    maxiters: int = 50
    tol: Optional[float] = None
    rtol: Optional[float] = None
    max_width: int = 256
    max_refine: int = 1


@dataclass
class Ros3:
    """DifferentialRiccatiEquations.jl:61 (dense only: X0 must be a matrix, inner_alg MatrixSign())"""
    inner_alg: Optional[MatrixSign] = None


@dataclass
class Ros4:
    """DifferentialRiccatiEquations.jl:62 (dense only: X0 must be a matrix, inner_alg MatrixSign())"""
    inner_alg: Optional[MatrixSign] = None


class Callbacks:
    """Observer hooks (src/Callbacks.jl:97-187).  The loop is device resident, so the per-iteration hooks are
    replayed in order after each Lyapunov solve with the recorded norms / shifts; `X` and `residual` are None
    for intermediate iterations."""
    NAMES = ("observe_gale_start", "observe_gale_step", "observe_gale_done", "observe_gale_failed",
             "observe_gale_metadata", "observe_gdre_start", "observe_gdre_step", "observe_gdre_done")


def _call(obs, name, *args):
    if obs is not None and hasattr(obs, name):
        getattr(obs, name)(*args)


_pencil_cache: dict = {}


def _pencil_for(E, A, ctx):
    key = (id(E), id(A), id(ctx))
    hit = _pencil_cache.get(key)
    if hit is not None and hit[0] is E and hit[1] is A:
        return hit[2]
    P = dev.Pencil(E, A, ctx)
    if len(_pencil_cache) > 8:
        _pencil_cache.clear()
    _pencil_cache[key] = (E, A, P)
    return P


def _split_operator(E, A):
    """GALE coefficient -> (sparse part, cA, cE, low-rank triple) with F = cA*A0 + cE*E + inv(alpha) U V."""
    if isinstance(A, LowRankUpdate):
        return A.A, (A.alpha, A.U, A.V)
    return A, None


@dataclass
class ScaledPencil:
    """`cA*A + cE*E` held lazily on the pencil of (E, A): the sparse part of the Rosenbrock operators (lowrank_ros1.jl:39 `A - E/(2τ)`,
    lowrank_ros2.jl:41 `γτA - E/2`).  The library takes the two coefficients directly (dre_adi_init cA, cE), so a time loop driven from
    the host re-uses ONE symbolic analysis instead of building a new sparse matrix and pencil per step."""
    A: Any
    cA: float
    E: Any
    cE: float

    @property
    def shape(self):
        return self.A.shape

    def tocsc(self):
        return (self.cA * self.A + self.cE * self.E).tocsc()


def _needs_state(observer) -> bool:
    """Observers that look at `X` / `residual` of intermediate ADI iterations (observe_gale_step!, adi.jl:119, Callbacks.jl:97-107) say so
    with a truthy attribute `needs_state`: the solve is then driven through the stepwise protocol and every call gets LDLᵀ handles that
    materialise on first access.  Without it the loop stays device resident and the hooks are replayed with norms and shifts only."""
    return observer is not None and bool(getattr(observer, "needs_state", False))


def _gale_operands(prob, ctx):
    """(pencil, cA, cE, sparse part as a matrix-like, low-rank triple) of a GALE coefficient."""
    A0, lr = _split_operator(prob.E, prob.A)
    if isinstance(A0, ScaledPencil):
        if A0.E is not prob.E:
            raise ValueError("ScaledPencil: E must be the GALE's own E")
        return _pencil_for(prob.E, A0.A, ctx), float(A0.cA), float(A0.cE), A0, lr
    return _pencil_for(prob.E, A0, ctx), 1.0, 0.0, A0, lr


def _callback_errors(keep):
    """Exceptions caught inside the ctypes trampolines of a call (user block solver, user shift strategy): they cannot cross the C boundary, the
    library reports DRE_ERR_INTERNAL, and the Python mirror chains the original exception to the DREError it raises."""
    out = []
    if isinstance(keep, (tuple, list)):
        for k in keep:
            if isinstance(k, list) and k and all(isinstance(e, BaseException) for e in k):
                out.extend(k)
            elif isinstance(k, (tuple, list)):
                out.extend(_callback_errors(k))
    return out


def _chk_with_callbacks(ctx, rc, keep):
    try:
        ctx.chk(rc)
    except DREError as e:
        errs = _callback_errors(keep)
        if errs:
            raise e from errs[0]
        raise


def _adi_options(alg: ADI, pencil, lr=None, E=None, A0=None):
    kind, nh, vals = _resolve_shifts(alg.shifts, pencil, lr)
    cb, keep_cb = _inner_solver_callback(getattr(alg, "inner_alg", None), E, A0) if E is not None else (None, None)
    opt, keep = _make_adi_options(alg, kind, nh, vals)
    if cb is not None:
        opt.inner_solve = C.cast(cb, C.c_void_p)
        keep = (keep, keep_cb)
    if kind == 3:
        scb, keep_scb = _shift_callback(alg.shifts, (E, A0))
        opt.shift_fn = C.cast(scb, C.c_void_p)
        keep = (keep, keep_scb)
    return opt, keep


def _make_adi_options(alg, kind, nh, vals):
    return dev.make_adi_options(alg.maxiters, alg.reltol, alg.abstol, alg.ignore_initial_guess, alg.compression_interval,
                                alg.compression, kind, nh, vals if kind == 0 else None, compress_exact=alg.compress_exact,
                                heuristic=vals if kind == 2 else None)


def _replay_gale(observer, prob, alg, info):
    _call(observer, "observe_gale_start", prob, alg)
    shifts = info["shifts"]
    pos = 0
    for it, nrm in zip(info["norm_iters"], info["norms"]):
        while pos < it:
            _call(observer, "observe_gale_metadata", "ADI shifts", shifts[pos])
            pos += 1
        _call(observer, "observe_gale_step", int(it), None, None, float(nrm))
    if not info["converged"]:
        _call(observer, "observe_gale_failed")


WARN_NOT_CONVERGED, WARN_ZERO_INCREMENT, WARN_RITZ_DISCARDED, WARN_RITZ_FLIPPED, WARN_PIVOT_GROWTH = 1, 2, 4, 8, 16      # include/dre_hip.h


def _adi_result_info(ctx, rptr):
    lib = ctx.lib
    ii = (C.c_int64 * 5)()
    dd = (C.c_double * 3)()
    lib.dre_adi_result_info(rptr, ii, dd)
    nn, iters = ii[3], ii[0]
    norms = np.zeros(nn)
    nit = np.zeros(nn, dtype=np.int32)
    sre, sim = np.zeros(max(iters, 1)), np.zeros(max(iters, 1))
    lib.dre_adi_result_history(rptr, norms.ctypes.data_as(C.POINTER(C.c_double)), nit.ctypes.data_as(C.POINTER(C.c_int32)),
                               sre.ctypes.data_as(C.POINTER(C.c_double)), sim.ctypes.data_as(C.POINTER(C.c_double)))
    return dict(iters=iters, converged=bool(ii[1]), warnings=ii[2], rhs_cols=ii[4], res_norm=dd[0], abstol=dd[1],
                initial_norm=dd[2], norms=norms, norm_iters=nit, shifts=(sre + 1j * sim)[:iters])


def solve_gale(prob: GALEProblem, alg: ADI, initial_guess: LDLt | None = None, observer=None, ctx=None, return_info=False):
    """solve(::GALEProblem{<:LDLᵀ}, ::ADI; initial_guess, observer)  (adi.jl:29-89)"""
    ctx = ctx or dev.default_context()
    if _needs_state(observer):
        # the observer wants X / residual of every iteration: stepwise protocol with live hooks (same bits as the one-shot solve)
        solver = ADISolver(prob, alg, initial_guess, observer, ctx)
        X = solver.solve()
        info = solver.info
        if not info["converged"] and alg.warn_convergence:
            warnings.warn(f"ADI did not converge: residual={info['res_norm']} abstol={info['abstol']} maxiters={alg.maxiters}")
        return (X, info) if return_info else X
    pencil, cA, cE, A0, lr = _gale_operands(prob, ctx)
    opt, keep = _adi_options(alg, pencil, lr, prob.E, A0)
    Cd = prob.C._to_device(ctx, pencil)
    X0d = initial_guess._to_device(ctx, pencil) if initial_guess is not None else None
    U = Vt = None
    alpha = 1.0
    if lr is not None:
        alpha, Uh, Vh = lr
        U, Vt = ctx.upload(Uh), ctx.upload(np.asarray(Vh).T)
    r = C.c_void_p()
    _chk_with_callbacks(ctx, ctx.lib.dre_gale_solve(ctx.ptr, pencil.ptr, cA, cE, float(alpha), U.ptr if U else None, Vt.ptr if Vt else None,
                                                     Cd.ptr, X0d.ptr if X0d else None, C.byref(opt), C.byref(r)), keep)
    try:
        info = _adi_result_info(ctx, r)
        xp = C.c_void_p()
        ctx.lib.dre_adi_result_take_x(r, C.byref(xp))
        X = LDLt([], [], [], _handle=dev.DeviceLDLt(ctx, xp, pencil))
    finally:
        ctx.lib.dre_adi_result_free(r)
    _replay_gale(observer, prob, alg, info)
    _call(observer, "observe_gale_done", info["iters"], X, None, info["res_norm"])
    if info["warnings"] & WARN_ZERO_INCREMENT:
        warnings.warn("Increment is zero")                      # adi.jl:201 (the iteration collapsed: isdone, adi.jl:134-137)
    if not info["converged"] and alg.warn_convergence and info["iters"] >= alg.maxiters:
        warnings.warn(f"ADI did not converge: residual={info['res_norm']} abstol={info['abstol']} maxiters={alg.maxiters}")
    elif not info["converged"] and alg.warn_convergence and not (info["warnings"] & WARN_ZERO_INCREMENT):
        warnings.warn(f"ADI did not converge: residual={info['res_norm']} abstol={info['abstol']} maxiters={alg.maxiters}")
    return (X, info) if return_info else X


class ADISolver:
    """The reference's `ADICache` protocol (src/lyapunov/adi.jl:5-21,91-141) on the device: `init(prob, alg)` -> solver, `step_(solver)` (one
    shift or one conjugate pair), `isdone(solver)`, `solve_(solver)`; iterating the solver steps it (`Base.iterate`, adi.jl:91-95).
    `X` materialises the current result (final compression included once the solve is done, adi.jl:78-80)."""

    def __init__(self, prob, alg, initial_guess=None, observer=None, ctx=None):
        self.ctx = ctx or dev.default_context()
        self.prob, self.alg, self.observer = prob, alg, observer
        self.pencil, cA, cE, A0, lr = _gale_operands(prob, self.ctx)
        opt, self._keep = _adi_options(alg, self.pencil, lr, prob.E, A0)
        self._live = _needs_state(observer)
        self._seen = 0                      # shifts already reported to a live observer
        self._Cd = prob.C._to_device(self.ctx, self.pencil)
        self._X0d = initial_guess._to_device(self.ctx, self.pencil) if initial_guess is not None else None
        self._U = self._Vt = None
        alpha = 1.0
        if lr is not None:
            alpha, Uh, Vh = lr
            self._U, self._Vt = self.ctx.upload(Uh), self.ctx.upload(np.asarray(Vh).T)
        self._ptr = C.c_void_p()
        self.ctx.chk(self.ctx.lib.dre_adi_init(self.ctx.ptr, self.pencil.ptr, cA, cE, float(alpha), self._U.ptr if self._U else None,
                                               self._Vt.ptr if self._Vt else None, self._Cd.ptr, self._X0d.ptr if self._X0d else None,
                                               C.byref(opt), C.byref(self._ptr)))
        self._result = None
        if self._live:                      # adi.jl:37,65: start, then the initial state as "step 0"
            _call(observer, "observe_gale_start", prob, alg)
            X, R = self.snapshot()
            _call(observer, "observe_gale_step", 0, X, R, self.state()["res_norm"])

    def snapshot(self):
        """(X, residual) of the current iteration as LDLᵀ handles (dre_adi_snapshot; adi.jl:119).  Nothing is downloaded until a handle is
        looked at (`rank()` and `norm` never download)."""
        xp, rp = C.c_void_p(), C.c_void_p()
        self.ctx.chk(self.ctx.lib.dre_adi_snapshot(self.ctx.ptr, self._ptr, C.byref(xp), C.byref(rp)))
        return (LDLt([], [], [], _handle=dev.DeviceLDLt(self.ctx, xp, self.pencil)),
                LDLt([], [], [], _handle=dev.DeviceLDLt(self.ctx, rp, self.pencil)))

    def _shifts_since(self, start):
        cnt = C.c_int64(0)
        self.ctx.lib.dre_adi_shifts(self._ptr, int(start), C.byref(cnt), None, None)
        re, im = np.zeros(max(cnt.value, 1)), np.zeros(max(cnt.value, 1))
        self.ctx.lib.dre_adi_shifts(self._ptr, int(start), C.byref(cnt), re.ctypes.data_as(C.POINTER(C.c_double)), im.ctypes.data_as(C.POINTER(C.c_double)))
        return [complex(a, b) if b != 0.0 else float(a) for a, b in zip(re[:cnt.value], im[:cnt.value])]

    def __del__(self):
        try:
            if getattr(self, "_ptr", None):
                self.ctx.lib.dre_adi_free(self._ptr)
                self._ptr = None
        except Exception:
            pass

    def isdone(self) -> bool:
        d = C.c_int()
        self.ctx.lib.dre_adi_isdone(self._ptr, C.byref(d))
        return bool(d.value)

    def state(self):
        it, rn, at = C.c_int64(), C.c_double(), C.c_double()
        self.ctx.lib.dre_adi_state(self._ptr, C.byref(it), C.byref(rn), C.byref(at))
        return dict(iters=it.value, res_norm=rn.value, abstol=at.value)

    def step(self):
        _chk_with_callbacks(self.ctx, self.ctx.lib.dre_adi_step(self.ctx.ptr, self._ptr), self._keep)
        if self._live:                      # adi.jl:103,119,192: the shift(s) of this step, then the step itself with its state
            st = self.state()
            for mu in self._shifts_since(self._seen):
                _call(self.observer, "observe_gale_metadata", "ADI shifts", mu)
            if st["iters"] > self._seen:
                X, R = self.snapshot()
                self._last_R = R                # adi.jl:84-87 hands residual(cache) to observe_gale_done! as well
                _call(self.observer, "observe_gale_step", int(st["iters"]), X, R, st["res_norm"])
            self._seen = st["iters"]
        return self

    def solve(self):
        if self._live:
            while not self.isdone():
                self.step()
        else:
            _chk_with_callbacks(self.ctx, self.ctx.lib.dre_adi_solve(self.ctx.ptr, self._ptr), self._keep)
        return self.X

    def __iter__(self):
        while not self.isdone():
            yield self.step()

    def _finish(self):
        if self._result is None:
            r = C.c_void_p()
            self.ctx.chk(self.ctx.lib.dre_adi_finish(self.ctx.ptr, self._ptr, C.byref(r)))
            try:
                info = _adi_result_info(self.ctx, r)
                xp = C.c_void_p()
                self.ctx.lib.dre_adi_result_take_x(r, C.byref(xp))
                X = LDLt([], [], [], _handle=dev.DeviceLDLt(self.ctx, xp, self.pencil))
            finally:
                self.ctx.lib.dre_adi_result_free(r)
            self._result = (X, info)
            if self._live:
                if not info["converged"]:
                    _call(self.observer, "observe_gale_failed")
                R = getattr(self, "_last_R", None)        # the residual object after the last iteration (a copy: dre_adi_snapshot)
                if R is None:
                    try:
                        _, R = self.snapshot()             # no iteration ran (converged at once): the initial residual
                    except Exception:
                        R = None
            else:
                _replay_gale(self.observer, self.prob, self.alg, info)
                R = None
            _call(self.observer, "observe_gale_done", info["iters"], X, R, info["res_norm"])
        return self._result

    @property
    def X(self) -> LDLt:
        if not self.isdone():
            raise RuntimeError("the iterate is device resident while the solve is running: finish it first (solve_ / step_ until isdone)")
        return self._finish()[0]

    @property
    def info(self):
        return self._finish()[1]


def init(prob, alg, initial_guess=None, observer=None, ctx=None) -> ADISolver:
    """CommonSolve.init(::GALEProblem{<:LDLᵀ}, ::ADI; initial_guess, observer)  (adi.jl:29-69)"""
    return ADISolver(prob, alg, initial_guess, observer, ctx)


def step_(solver: ADISolver) -> ADISolver:
    """step!(cache)  (adi.jl:97-128)"""
    return solver.step()


def isdone(solver: ADISolver) -> bool:
    """isdone(cache)  (adi.jl:130-141)"""
    return solver.isdone()


def solve_(solver: ADISolver) -> LDLt:
    """solve!(cache)  (adi.jl:71-89)"""
    return solver.solve()


def residual(prob, X: LDLt, ctx=None) -> LDLt:
    """residual(::GALEProblem{<:LDLᵀ}, ::LDLᵀ)  (lyapunov/residual.jl:3-31);  residual(::GAREProblem, ::LDLᵀ)  (riccati/residual.jl:5-52);
    residual(::GAREProblem, ::ndarray): the dense residual as an ndarray (riccati/residual.jl:54-66, gare_residual_dense)"""
    if isinstance(prob, GAREProblem):
        if isinstance(X, LDLt):
            return gare_residual(prob, X, ctx)
        if isinstance(X, np.ndarray):
            return gare_residual_dense(prob, X, ctx)
        raise TypeError(f"residual(GAREProblem, X): X must be an LDLᵀ object or a dense ndarray, not {type(X).__name__}")
    ctx = ctx or dev.default_context()
    A0, lr = _split_operator(prob.E, prob.A)
    pencil = _pencil_for(prob.E, A0, ctx)
    Cd = prob.C._to_device(ctx, pencil)
    Xd = X._to_device(ctx, pencil)
    U = Vt = None
    alpha = 1.0
    if lr is not None:
        alpha, Uh, Vh = lr
        U, Vt = ctx.upload(Uh), ctx.upload(np.asarray(Vh).T)
    out = C.c_void_p()
    ctx.chk(ctx.lib.dre_gale_residual(ctx.ptr, pencil.ptr, 1.0, 0.0, float(alpha), U.ptr if U else None, Vt.ptr if Vt else None,
                                      Cd.ptr, Xd.ptr, C.byref(out)))
    return LDLt([], [], [], _handle=dev.DeviceLDLt(ctx, out, pencil))


def _check_adaptive(prob, alg, dt, adaptive):
    """the argument errors of adaptive= (raised before any device work)"""
    if not isinstance(adaptive, StepControl):
        raise TypeError("adaptive= takes a StepControl(...) object")
    if isinstance(prob.X0, LDLt):
        raise TypeError("adaptive= (step-size control) exists for the dense path only: it needs a dense X0 (an ndarray), not an LDLᵀ object; "
                        "nothing was run on the device")
    if not isinstance(alg, Ros2):
        raise TypeError(f"adaptive= (step-size control) exists for Ros2 only, not {type(alg).__name__}: Ros2's embedded first-order solution is "
                        "the error estimator; nothing was run on the device")
    if not isinstance(alg.inner_alg, MatrixSign):
        raise TypeError("adaptive= (step-size control) runs with the inner algorithm MatrixSign() named explicitly, Ros2(MatrixSign()); "
                        "nothing was run on the device")
    t0, tf = float(prob.tspan[0]), float(prob.tspan[1])
    dt0 = float(dt)
    bad = None
    if not (math.isfinite(t0) and math.isfinite(tf) and tf != t0):
        bad = "tspan must have two finite, different ends"
    elif not (math.isfinite(dt0) and dt0 != 0.0 and (dt0 > 0) == (tf > t0)):
        bad = "dt (the first step) must be finite, nonzero and of the sign of tspan[1] - tspan[0]"
    elif not (adaptive.rtol > 0 and math.isfinite(adaptive.rtol)):
        bad = "rtol must be positive"
    elif not (adaptive.atol > 0 and math.isfinite(adaptive.atol)):
        bad = "atol must be positive (with atol = 0 a zero entry of X has no error scale)"
    elif not (0 <= adaptive.dt_min <= adaptive.dt_max):
        bad = "0 <= dt_min <= dt_max expected"
    elif int(adaptive.max_steps) < 1:
        bad = "max_steps must be >= 1"
    else:
        prev = t0
        for s_ in adaptive.tstops:
            s_ = float(s_)
            if not ((prev < s_ < tf) if tf > t0 else (prev > s_ > tf)):
                bad = "tstops must lie strictly between the ends of tspan and be strictly monotone in the direction of integration"
                break
            prev = s_
    if bad:
        raise ValueError(f"adaptive=: {bad}; nothing was run on the device")


def solve_gdre(prob: GDREProblem, alg, dt, save_state=False, observer=None, ctx=None, return_stats=False, adaptive=None):
    """solve(::GDREProblem{<:LDLᵀ}, ::Ros1/Ros2; dt, save_state, observer)
    (DifferentialRiccatiEquations.jl:78-94, riccati/lowrank_ros1.jl, lowrank_ros2.jl)
    adaptive=StepControl(...): Ros2(MatrixSign()) with a dense X0 under step-size control, dt being the first step (_solve_gdre_dense)."""
    if adaptive is not None:
        _check_adaptive(prob, alg, dt, adaptive)
        return _solve_gdre_dense(prob, alg, 2, dt, save_state, observer, ctx, return_stats, adaptive=adaptive)
    dense_order = {Ros1: 1, Ros2: 2, Ros3: 3, Ros4: 4}.get(type(alg))
    if not isinstance(prob.X0, LDLt):
        if isinstance(getattr(alg, "inner_alg", None), FactoredSign):
            raise TypeError("FactoredSign() is a low-rank solver: it needs an LDLᵀ X0; a dense X0 (an ndarray) goes with MatrixSign()")
        if dense_order is None or not isinstance(alg.inner_alg, MatrixSign):
            raise TypeError("a dense X0 selects the dense Rosenbrock methods, which run on the device only with the matrix-sign-function solver "
                            "named explicitly, e.g. Ros1(MatrixSign()): it needs a c-stable pencil, unlike the reference's Bartels-Stewart default")
        return _solve_gdre_dense(prob, alg, dense_order, dt, save_state, observer, ctx, return_stats)
    if isinstance(alg, (Ros3, Ros4)):
        raise TypeError("Ros3 and Ros4 have no low-rank formulation: X0 must be a dense matrix")
    order = 1 if isinstance(alg, Ros1) else 2 if isinstance(alg, Ros2) else None
    if order is None:
        raise TypeError("only Ros1 and Ros2 have a low-rank formulation")
    if isinstance(alg.inner_alg, MatrixSign):
        raise TypeError("MatrixSign() is a dense solver: it needs a dense X0 (an ndarray), not an LDLᵀ object")
    ctx = ctx or dev.default_context()
    if isinstance(alg.inner_alg, FactoredSign):
        return _solve_gdre_factored_sign(prob, alg, order, alg.inner_alg, dt, save_state, observer, ctx, return_stats)
    inner = alg.inner_alg if alg.inner_alg is not None else ADI()
    if _needs_state(observer):
        return _solve_gdre_observed(prob, alg, order, inner, dt, save_state, observer, ctx, return_stats)
    _call(observer, "observe_gdre_start", prob, alg)
    _t0 = time.perf_counter()
    pencil = _pencil_for(prob.E, prob.A, ctx)
    opt, keep = _adi_options(inner, pencil, None, prob.E, prob.A)
    X0d = prob.X0._to_device(ctx, pencil)
    Bd, Cd = ctx.upload(prob.B), ctx.upload(prob.C)
    r = C.c_void_p()
    _t1 = time.perf_counter()
    _chk_with_callbacks(ctx, ctx.lib.dre_gdre_solve(ctx.ptr, pencil.ptr, Bd.ptr, Cd.ptr, X0d.ptr, float(prob.tspan[0]), float(prob.tspan[1]),
                                   float(dt), order, int(bool(save_state)), C.byref(opt), C.byref(r)), keep)
    _t2 = time.perf_counter()
    lib = ctx.lib
    try:
        ii = (C.c_int64 * 7)()
        lib.dre_gdre_result_info(r, ii)
        nt, nx, iters, nfac, ngale, m, n = list(ii)
        t = np.zeros(nt)
        lib.dre_gdre_result_times(r, t.ctypes.data_as(C.POINTER(C.c_double)))
        Kall = np.zeros((nt, n, m))            # block i = K(t_i), m x n column-major: one export launch + one copy for the whole trajectory
        ctx.chk(lib.dre_gdre_result_K_all(ctx.ptr, r, Kall.ctypes.data_as(C.POINTER(C.c_double))))
        Ks = [Kall[i].T for i in range(nt)]
        Xs = [prob.X0]                    # first(sol.X) === prob.X0  (test/rail.jl:40)
        for i in range(1, nx):
            xp = C.c_void_p()
            lib.dre_gdre_result_X(r, i, C.byref(xp))
            Xs.append(LDLt([], [], [], _handle=dev.DeviceLDLt(ctx, xp, pencil)))
        gales = []
        if ngale:
            pd, pi64, pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
            gi, gd = np.zeros((ngale, 6), dtype=np.int64), np.zeros((ngale, 2))
            lib.dre_gdre_result_gales_all(r, gi.ctypes.data_as(pi64), gd.ctypes.data_as(pd), None, None, None, None)
            nn, ns = int(gi[:, 4].sum()), int(gi[:, 5].sum())
            norms, nit = np.zeros(max(nn, 1)), np.zeros(max(nn, 1), dtype=np.int32)
            sre, sim = np.zeros(max(ns, 1)), np.zeros(max(ns, 1))
            lib.dre_gdre_result_gales_all(r, None, None, norms.ctypes.data_as(pd), nit.ctypes.data_as(pi32), sre.ctypes.data_as(pd), sim.ctypes.data_as(pd))
            shifts = sre + 1j * sim
            on = os_ = 0
            for j in range(ngale):
                cn, cs = int(gi[j, 4]), int(gi[j, 5])
                gales.append(dict(iters=int(gi[j, 0]), converged=bool(gi[j, 1]), warnings=int(gi[j, 2]), rhs_cols=int(gi[j, 3]), res_norm=float(gd[j, 0]),
                                  abstol=float(gd[j, 1]), norms=norms[on:on + cn], norm_iters=nit[on:on + cn], shifts=shifts[os_:os_ + cs]))
                on += cn; os_ += cs
    finally:
        lib.dre_gdre_result_free(r)
    _t3 = time.perf_counter()
    per_step = ngale // max(nt - 1, 1) if nt > 1 else 0
    _call(observer, "observe_gdre_step", t[0], Xs[0], Ks[0])
    for i in range(1, nt):
        for g in gales[(i - 1) * per_step:i * per_step]:
            # per-iteration hooks in the order of adi.jl:37,65,103,119,192: the loop ran device resident, so X and the residual object of
            # the intermediate iterations are not materialised (None); the norms and shifts are the recorded ones
            _replay_gale(observer, None, inner, g)
            _call(observer, "observe_gale_done", g["iters"], None, None, g["res_norm"])
            if not g["converged"]:
                if inner.warn_convergence:
                    warnings.warn(f"ADI did not converge: residual={g['res_norm']} abstol={g['abstol']} maxiters={inner.maxiters}")
        Xi = Xs[i] if save_state else (Xs[-1] if i == nt - 1 else None)
        _call(observer, "observe_gdre_step", t[i], Xi, Ks[i])
    _call(observer, "observe_gdre_done")
    sol = DRESolution(Xs, Ks, t)
    if return_stats:
        return sol, dict(adi_iters=iters, factorizations=nfac, gales=gales,
                         host_ms=dict(upload=(_t1 - _t0) * 1e3, solve=(_t2 - _t1) * 1e3, results=(_t3 - _t2) * 1e3, hooks=(time.perf_counter() - _t3) * 1e3))
    return sol


# ------------------------------------------------------------------------------------------------
# Dense path                                 src/riccati/dense_ros{1,2,3,4}.jl, src/lyapunov/bartels-stewart.jl
# ------------------------------------------------------------------------------------------------
def _dense_f64(M):
    M = M.toarray() if sp.issparse(M) else np.asarray(M, dtype=float)       # collect(E) (dense_ros1.jl:16)
    return np.asfortranarray(M, dtype=float)


def _sign_params(alg: MatrixSign):
    return int(alg.maxiters), float(alg.tol) if alg.tol is not None else 0.0, int(alg.max_refine)


def solve_gale_dense(prob: GALEProblem, alg: MatrixSign, ctx=None, return_info=False):
    """solve(::GALEProblem, ::MatrixSign): A'XE + E'XA = -C with dense X (bartels-stewart.jl:3-12, lyapc replaced by the sign iteration).
    C may be an ndarray or an LDLᵀ object (densified as bartels-stewart.jl:6-8 does)."""
    Cm = prob.C.dense() if isinstance(prob.C, LDLt) else prob.C
    E, A, Cm = _dense_f64(prob.E), _dense_f64(prob.A), _dense_f64(Cm)
    ctx = ctx or dev.default_context()
    Ed, Ad, Cd = ctx.upload(E), ctx.upload(A), ctx.upload(Cm)
    xp = C.c_void_p()
    ii, dd = (C.c_int64 * 2)(), (C.c_double * 2)()
    maxiters, tol, max_refine = _sign_params(alg)
    ctx.chk(ctx.lib.dre_dense_gale_solve(ctx.ptr, Ed.ptr, Ad.ptr, Cd.ptr, maxiters, tol, max_refine, C.byref(xp), ii, dd))
    X = dev.DenseMatrix(ctx, xp).numpy()
    if return_info:
        return X, dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1]))
    return X


def dense_invert(A, ctx=None):
    """inv(A) by the device's in-place Gauss-Jordan inversion (dre_dense_invert) with the context's pivoting panel (option dense_gj_panel):
    (Ainv, piv, logabsdet).  piv holds the row interchanges, LAPACK style with 0-based indices (row j was swapped with row piv[j] >= j);
    logabsdet = log |det A|.  A singular A raises DREError(-4)."""
    A = _dense_f64(A)
    ctx = ctx or dev.default_context()
    Ad = ctx.upload(A)
    n = A.shape[0]
    piv = np.zeros(n, dtype=np.int32)
    ld = C.c_double()
    ctx.chk(ctx.lib.dre_dense_invert(ctx.ptr, Ad.ptr, piv.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ld)))
    return Ad.numpy(), piv, float(ld.value)


def _solve_gdre_dense(prob, alg, order, dt, save_state, observer, ctx, return_stats, adaptive=None):
    """solve(::GDREProblem{<:Matrix}, ::Ros<order>(MatrixSign()); dt, save_state, observer)  (dense_ros{1,2,3,4}.jl), device resident;
    the observer hooks are replayed afterwards in dense_ros1.jl's order.  adaptive (a StepControl): Ros2 under step-size control
    (dre_dense_gdre_solve_adaptive); the solution's t is the non-uniform grid of the accepted steps, which are all the observer sees, and
    return_stats adds accepted, rejected and err (one value per accepted step)."""
    ctx = ctx or dev.default_context()
    E, A, X0 = _dense_f64(prob.E), _dense_f64(prob.A), _dense_f64(prob.X0)
    Bm, Cm = _dense_f64(prob.B), _dense_f64(prob.C)
    ups = [ctx.upload(M) for M in (E, A, Bm, Cm, X0)]
    maxiters, tol, max_refine = _sign_params(alg.inner_alg)
    r = C.c_void_p()
    lib = ctx.lib
    if adaptive is not None:
        ts = np.array([float(s_) for s_ in adaptive.tstops], dtype=float)
        ctx.chk(lib.dre_dense_gdre_solve_adaptive(ctx.ptr, *[u.ptr for u in ups], float(prob.tspan[0]), float(prob.tspan[1]), float(dt), int(order),
                                                  float(adaptive.rtol), float(adaptive.atol), float(adaptive.dt_min), float(adaptive.dt_max),
                                                  int(adaptive.max_steps), ts.ctypes.data_as(C.POINTER(C.c_double)), len(ts),
                                                  int(bool(save_state)), maxiters, tol, max_refine, C.byref(r)))
    else:
        ctx.chk(lib.dre_dense_gdre_solve(ctx.ptr, *[u.ptr for u in ups], float(prob.tspan[0]), float(prob.tspan[1]), float(dt), int(order),
                                         int(bool(save_state)), maxiters, tol, max_refine, C.byref(r)))
    try:
        ii = (C.c_int64 * 7)()
        lib.dre_gdre_result_info(r, ii)
        nt, nx, _, _, nsolve, m, n = list(ii)
        t = np.zeros(nt)
        lib.dre_gdre_result_times(r, t.ctypes.data_as(C.POINTER(C.c_double)))
        Kall = np.zeros((nt, n, m))
        ctx.chk(lib.dre_gdre_result_K_all(ctx.ptr, r, Kall.ctypes.data_as(C.POINTER(C.c_double))))
        Ks = [Kall[i].T for i in range(nt)]
        Xs = [prob.X0]                    # first(sol.X) === prob.X0  (test/rail.jl:40)
        for i in range(1, nx):
            xp = C.c_void_p()
            ctx.chk(lib.dre_gdre_result_X_dense(ctx.ptr, r, i, C.byref(xp)))
            Xs.append(dev.DenseMatrix(ctx, xp).numpy())
        its, refs = np.zeros(max(nsolve, 1), dtype=np.int64), np.zeros(max(nsolve, 1), dtype=np.int64)
        res = np.zeros(2 * max(nsolve, 1))
        lib.dre_gdre_result_dense_stats(r, its.ctypes.data_as(C.POINTER(C.c_int64)), refs.ctypes.data_as(C.POINTER(C.c_int64)),
                                        res.ctypes.data_as(C.POINTER(C.c_double)))
        if adaptive is not None:
            counts, errs = (C.c_int64 * 2)(), np.zeros(max(nt - 1, 1))
            lib.dre_gdre_result_step_stats(r, counts, errs.ctypes.data_as(C.POINTER(C.c_double)))
    finally:
        lib.dre_gdre_result_free(r)
    _call(observer, "observe_gdre_start", prob, alg)
    for i in range(nt):
        Xi = Xs[i] if (save_state or i == 0) else (Xs[-1] if i == nt - 1 else None)
        _call(observer, "observe_gdre_step", t[i], Xi, Ks[i])
    _call(observer, "observe_gdre_done")
    sol = DRESolution(Xs, Ks, t)
    if return_stats:
        solves = [dict(iters=int(its[j]), refinements=int(refs[j]), res0=float(res[2 * j]), res=float(res[2 * j + 1])) for j in range(nsolve)]
        stats = dict(lyapunov_solves=nsolve, solves=solves)
        if adaptive is not None:
            stats.update(accepted=int(counts[0]), rejected=int(counts[1]), err=errs[:nt - 1].copy())
        return sol, stats
    return sol


# ------------------------------------------------------------------------------------------------
# Batched dense path: an ensemble of same-size problems in shared launches                       csrc/dense_batch.hip
# ------------------------------------------------------------------------------------------------
def _handle_array(objs):
    return (C.c_void_p * len(objs))(*[o.ptr for o in objs])


def _batch_errors(ctx, status):
    """DREError per failed member of the last batched call (None for the others)"""
    errs = []
    for b, code in enumerate(status):
        if code == 0:
            errs.append(None)
        else:
            msg = ctx.lib.dre_batch_member_error(ctx.ptr, b)
            errs.append(DREError(int(code), msg.decode() if msg else f"member {b} failed"))
    return errs


def _check_batch(probs, alg, observer):
    """The argument errors of solve_batch, raised before any device call: -> ("gale" | "gdre" | "gare", order)"""
    if observer is not None:
        raise TypeError("solve_batch: observers are not supported in the batched call")
    probs = list(probs)
    if len(probs) == 0:
        raise ValueError("solve_batch: empty list of problems")
    if all(isinstance(p, GALEProblem) for p in probs):
        if not isinstance(alg, MatrixSign):
            raise TypeError("solve_batch: a list of GALEProblem is solved with MatrixSign()")
        kind, order = "gale", 0
    elif all(isinstance(p, GDREProblem) for p in probs):
        order = {Ros1: 1, Ros2: 2}.get(type(alg))
        if order is None or not isinstance(getattr(alg, "inner_alg", None), MatrixSign):
            raise TypeError("solve_batch: a list of GDREProblem is solved with Ros1(MatrixSign()) or Ros2(MatrixSign()); Ros3 and Ros4 are not batched")
        if any(isinstance(p.X0, LDLt) for p in probs):
            raise TypeError("solve_batch: the batched Rosenbrock methods are the dense ones, X0 must be a dense matrix")
        kind = "gdre"
    elif all(isinstance(p, GAREProblem) for p in probs):
        if not isinstance(alg, MatrixSign):
            raise TypeError("solve_batch: a list of GAREProblem is solved with MatrixSign()")
        kind, order = "gare", 0
    else:
        raise TypeError("solve_batch: the problems must be all GALEProblem, all GDREProblem or all GAREProblem")

    def shape(p):
        n = p.E.shape[0]
        if kind == "gale":
            return (n,)
        if kind == "gare":
            (_, Bm, _), (_, Ct, _) = p.G, p.Q
            return (n, np.shape(Bm)[1] if np.ndim(Bm) == 2 else 1, np.shape(Ct)[1] if np.ndim(Ct) == 2 else 1)
        return (n, np.asarray(p.B).shape[1] if np.ndim(p.B) == 2 else 1, np.asarray(p.C).shape[0] if np.ndim(p.C) == 2 else 1)

    s0 = shape(probs[0])
    for b, p in enumerate(probs):
        if shape(p) != s0:
            raise ValueError(f"solve_batch: member {b} has (n, m, q) = {shape(p)}, member 0 has {s0}: the members of a batch share n, m and q")
    if kind == "gdre" and any(tuple(p.tspan) != tuple(probs[0].tspan) for p in probs):
        raise ValueError("solve_batch: the members of a batch share tspan")
    return kind, order


def solve_batch(probs, alg, *, dt=None, save_state=False, errors="raise", ctx=None, return_stats=False, observer=None, adaptive=None):
    """An ensemble of independent problems of one size side by side on one device (dre_dense_gale_solve_batched /
    dre_dense_gdre_solve_batched / dre_dense_gare_solve_batched): a list of GALEProblem with MatrixSign(), of GDREProblem with dense X0
    with Ros1(MatrixSign()) / Ros2(MatrixSign()), or of GAREProblem with MatrixSign() (2n <= 4096; with return_stats the info dict of
    solve_gare_dense: iters, refinements, res0, res, K).  Returns the list of results in member order (what `solve` returns for each; with return_stats the pairs
    (result, stats)).  A member's result depends on that member's data only.  errors="raise": the first failed member's DREError (its message
    names the member); errors="return": the DREError object in that member's slot (a failed GDRE member's completed steps are in its
    `partial` attribute)."""
    if errors not in ("raise", "return"):
        raise ValueError('solve_batch: errors must be "raise" or "return"')
    if adaptive is not None:
        raise TypeError("solve_batch: adaptive= (step-size control) is not batched, the members of a batch share one fixed grid; solve the problems "
                        "one by one with solve(prob, Ros2(MatrixSign()), dt=dt0, adaptive=...); nothing was run on the device")
    probs = list(probs)
    kind, order = _check_batch(probs, alg, observer)
    if kind == "gdre" and dt is None:
        raise ValueError("solve_batch: dt is required for GDRE problems")
    if kind == "gare" and (dt is not None or save_state):
        raise ValueError("solve_batch: dt and save_state belong to GDRE problems, a list of GAREProblem takes neither")
    ctx = ctx or dev.default_context()
    nb = len(probs)
    status = np.zeros(nb, dtype=np.int32)
    pst = status.ctypes.data_as(C.POINTER(C.c_int32))
    lib = ctx.lib
    if kind == "gale":
        maxiters, tol, max_refine = _sign_params(alg)
        Es, Fs, Rs = [], [], []
        for p in probs:
            Cm = p.C.dense() if isinstance(p.C, LDLt) else p.C
            Es.append(ctx.upload(_dense_f64(p.E))); Fs.append(ctx.upload(_dense_f64(p.A))); Rs.append(ctx.upload(_dense_f64(Cm)))
        xs = (C.c_void_p * nb)()
        ii, dd = np.zeros(2 * nb, dtype=np.int64), np.zeros(2 * nb)
        ctx.chk(lib.dre_dense_gale_solve_batched(ctx.ptr, nb, _handle_array(Es), _handle_array(Fs), _handle_array(Rs), maxiters, tol, max_refine, xs,
                                                 ii.ctypes.data_as(C.POINTER(C.c_int64)), dd.ctypes.data_as(C.POINTER(C.c_double)), pst))
        errs = _batch_errors(ctx, status)
        out = []
        for b in range(nb):
            if errs[b] is not None:
                out.append(errs[b])
                continue
            X = dev.DenseMatrix(ctx, C.c_void_p(xs[b])).numpy()
            info = dict(iters=int(ii[2 * b]), refinements=int(ii[2 * b + 1]), res0=float(dd[2 * b]), res=float(dd[2 * b + 1]))
            out.append((X, info) if return_stats else X)
    elif kind == "gare":
        maxiters, tol, max_refine = _sign_params(alg)
        ops = [_gare_dense_operands(p, ctx) for p in probs]                          # (uploads kept alive, (E, A, B, Rinv, Ct, S) handles)
        arrs = [(C.c_void_p * nb)(*[o[1][j] for o in ops]) for j in range(6)]
        xs = (C.c_void_p * nb)()
        ii, dd = np.zeros(2 * nb, dtype=np.int64), np.zeros(2 * nb)
        rc = lib.dre_dense_gare_solve_batched(ctx.ptr, nb, *arrs, maxiters, tol, max_refine, xs, ii.ctypes.data_as(C.POINTER(C.c_int64)),
                                              dd.ctypes.data_as(C.POINTER(C.c_double)), pst)
        if rc != 0 and not status.any():                                             # the call's own error; a member's code comes with status
            ctx.chk(rc)
        del ops
        errs = _batch_errors(ctx, status)
        out = []
        for b, p in enumerate(probs):
            if errs[b] is not None:
                out.append(errs[b])
                continue
            X = dev.DenseMatrix(ctx, C.c_void_p(xs[b])).numpy()
            if return_stats:
                beta, Bm, Rinv = p.G
                E = p.E.toarray() if sp.issparse(p.E) else np.asarray(p.E, dtype=float)
                K = (beta * np.asarray(Rinv, dtype=float)) @ (np.asarray(Bm, dtype=float).T @ X @ E)
                out.append((X, dict(iters=int(ii[2 * b]), refinements=int(ii[2 * b + 1]), res0=float(dd[2 * b]), res=float(dd[2 * b + 1]), K=K)))
            else:
                out.append(X)
    else:
        maxiters, tol, max_refine = _sign_params(alg.inner_alg)
        ups = [[ctx.upload(_dense_f64(M)) for M in (p.E, p.A, p.B, p.C, p.X0)] for p in probs]
        rs = (C.c_void_p * nb)()
        p0 = probs[0]
        ctx.chk(lib.dre_dense_gdre_solve_batched(ctx.ptr, nb, *[_handle_array([u[j] for u in ups]) for j in range(5)], float(p0.tspan[0]),
                                                 float(p0.tspan[1]), float(dt), int(order), int(bool(save_state)), maxiters, tol, max_refine, rs, pst))
        errs = _batch_errors(ctx, status)
        out = []
        for b in range(nb):
            res = _dense_result(ctx, C.c_void_p(rs[b]), probs[b], return_stats)
            if errs[b] is not None:
                errs[b].partial = res
                out.append(errs[b])
            else:
                out.append(res)
    if errors == "raise":
        for e in out:
            if isinstance(e, DREError):
                raise e
    return out


def dense_invert_batch(As, ctx=None):
    """inv(A_b) for a list of square matrices of one order n <= 4096 in shared launches (dre_dense_invert_batched, the register panel):
    the list of (Ainv, piv, logabsdet) as `dense_invert` returns them.  A singular member raises DREError(-4) naming it."""
    As = [_dense_f64(A) for A in As]
    if len(As) == 0:
        raise ValueError("dense_invert_batch: empty list of matrices")
    n = As[0].shape[0]
    for b, A in enumerate(As):
        if A.shape != (n, n):
            raise ValueError(f"dense_invert_batch: member {b} has shape {A.shape}, expected ({n}, {n})")
    ctx = ctx or dev.default_context()
    nb = len(As)
    Ad = [ctx.upload(A) for A in As]
    piv, ld, status = np.zeros((nb, n), dtype=np.int32), np.zeros(nb), np.zeros(nb, dtype=np.int32)
    ctx.chk(ctx.lib.dre_dense_invert_batched(ctx.ptr, nb, _handle_array(Ad), piv.ctypes.data_as(C.POINTER(C.c_int32)),
                                             ld.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_int32))))
    for e in _batch_errors(ctx, status):
        if e is not None:
            raise e
    return [(Ad[b].numpy(), piv[b].copy(), float(ld[b])) for b in range(nb)]


COMPLEX_PANEL_MAX_N = 4096       # the complex register panel of csrc/dense_cgj.hip


def dense_invert_complex_batch(As, errors="raise", ctx=None):
    """inv(A_b) for a list of square complex matrices of one order n <= 4096 in shared launches (`dre_dense_invert_complex_batched`): the
    native complex Gauss-Jordan inversion on the register panel, pivoting by |re| + |im|, 8 n³ real flops and 2 n² doubles per member ->
    the list of (Ainv complex, piv, logabsdet = log|det A_b|).  A singular member (exactly zero or non-finite pivot) raises DREError(-4)
    naming it; errors="return" puts that DREError in the member's place and returns the others.  An empty list, a member that is not
    n x n and n > 4096 are errors before anything runs on the device."""
    name = "dense_invert_complex_batch"
    _batch_errors_arg(name, errors)
    As = [np.asarray(A, dtype=complex) for A in As]
    if len(As) == 0:
        raise ValueError(f"{name}: empty list of matrices; nothing was run on the device")
    n = As[0].shape[0] if As[0].ndim == 2 else -1
    for b, A in enumerate(As):
        if A.ndim != 2 or A.shape != (n, n) or n < 1:
            raise ValueError(f"{name}: member {b} has shape {A.shape}, expected a square matrix of the order of member 0; nothing was run on the device")
    if n > COMPLEX_PANEL_MAX_N:
        raise ValueError(f"{name}: the complex register panel inverts matrices of order n <= {COMPLEX_PANEL_MAX_N}; got n = {n}; nothing was run "
                         "on the device")
    ctx = ctx or dev.default_context()
    nb = len(As)
    Ar, Ai = [ctx.upload(_dense_f64(A.real)) for A in As], [ctx.upload(_dense_f64(A.imag)) for A in As]
    piv, ld, status = np.zeros((nb, n), dtype=np.int32), np.zeros(nb), np.zeros(nb, dtype=np.int32)
    ctx.chk(ctx.lib.dre_dense_invert_complex_batched(ctx.ptr, nb, _handle_array(Ar), _handle_array(Ai), piv.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     ld.ctypes.data_as(C.POINTER(C.c_double)), status.ctypes.data_as(C.POINTER(C.c_int32))))
    out = []
    for b, e in enumerate(_batch_errors(ctx, status)):
        if e is not None:
            if errors == "raise":
                raise e
            out.append(e)
        else:
            out.append((Ar[b].numpy() + 1j * Ai[b].numpy(), piv[b].copy(), float(ld[b])))
    return out


def dense_invert_complex(A, ctx=None):
    """inv(A) of a square complex matrix of order n <= 4096 by the device's complex Gauss-Jordan inversion (a batch of one of
    `dense_invert_complex_batch`) -> (Ainv complex, piv, logabsdet).  A singular matrix raises DREError(-4)."""
    A = np.asarray(A, dtype=complex)
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError(f"dense_invert_complex: a square matrix is expected, got shape {A.shape}; nothing was run on the device")
    return dense_invert_complex_batch([A], ctx=ctx)[0]


def _dense_result(ctx, r, prob, return_stats):
    """a dense dre_gdre_result handle -> DRESolution (or (DRESolution, stats)); frees the handle"""
    lib = ctx.lib
    try:
        ii = (C.c_int64 * 7)()
        lib.dre_gdre_result_info(r, ii)
        nt, nx, _, _, nsolve, m, n = list(ii)
        t = np.zeros(nt)
        lib.dre_gdre_result_times(r, t.ctypes.data_as(C.POINTER(C.c_double)))
        Kall = np.zeros((nt, n, m))
        ctx.chk(lib.dre_gdre_result_K_all(ctx.ptr, r, Kall.ctypes.data_as(C.POINTER(C.c_double))))
        Ks = [Kall[i].T for i in range(nt)]
        Xs = [prob.X0]
        for i in range(1, nx):
            xp = C.c_void_p()
            ctx.chk(lib.dre_gdre_result_X_dense(ctx.ptr, r, i, C.byref(xp)))
            Xs.append(dev.DenseMatrix(ctx, xp).numpy())
        its, refs = np.zeros(max(nsolve, 1), dtype=np.int64), np.zeros(max(nsolve, 1), dtype=np.int64)
        res = np.zeros(2 * max(nsolve, 1))
        lib.dre_gdre_result_dense_stats(r, its.ctypes.data_as(C.POINTER(C.c_int64)), refs.ctypes.data_as(C.POINTER(C.c_int64)),
                                        res.ctypes.data_as(C.POINTER(C.c_double)))
    finally:
        lib.dre_gdre_result_free(r)
    sol = DRESolution(Xs, Ks, t)
    if return_stats:
        solves = [dict(iters=int(its[j]), refinements=int(refs[j]), res0=float(res[2 * j]), res=float(res[2 * j + 1])) for j in range(nsolve)]
        return sol, dict(lyapunov_solves=nsolve, solves=solves)
    return sol


def _solve_gdre_observed(prob, alg, order, inner, dt, save_state, observer, ctx, return_stats):
    """The Rosenbrock time loop driven from the host for observers that look at the state of every ADI iteration
    (src/riccati/lowrank_ros1.jl:19-63, lowrank_ros2.jl:19-86): every Lyapunov solve is a device-resident stepwise solver
    (`ADISolver`) whose hooks fire live with (X, residual) handles; feedback, right-hand sides and their compression are the library's
    (`dre_ldlt_feedback`, `compress_`).  Same equations as the device-resident loop (`dre_gdre_solve`), which is what runs when the
    observer does not ask for state."""
    gales = []

    def step_solver(F):
        def lyap(rhs, guess):
            solver = ADISolver(GALEProblem(prob.E, F, rhs), inner, guess, observer, ctx)
            Xn = solver.solve()
            info = solver.info
            gales.append(info)
            if not info["converged"] and inner.warn_convergence:
                warnings.warn(f"ADI did not converge: residual={info['res_norm']} abstol={info['abstol']} maxiters={inner.maxiters}")
            return Xn
        return lyap

    sol = _rosenbrock_lowrank_loop(prob, alg, order, dt, save_state, observer, step_solver)
    if return_stats:
        return sol, dict(adi_iters=sum(g["iters"] for g in gales), factorizations=None, gales=gales)
    return sol


def _rosenbrock_lowrank_loop(prob, alg, order, dt, save_state, observer, step_solver):
    """Host-driven low-rank Ros1 / Ros2 loop shared by the inner Lyapunov solvers: `step_solver(F)` is called once per time step with the
    step's operator and returns `lyap(rhs, guess) -> LDLᵀ` for that step's stage solves."""
    E, A, B, Cm = prob.E, prob.A, np.asarray(prob.B, float), np.asarray(prob.C, float)
    q = Cm.shape[0]
    nsteps = int(np.floor((prob.tspan[1] - prob.tspan[0]) / dt + 1e-9))
    t = prob.tspan[0] + dt * np.arange(nsteps + 1)
    gamma = 1.0 + 1.0 / np.sqrt(2.0)
    _call(observer, "observe_gdre_start", prob, alg)

    def feedback(X):
        a, L, Dm = X                                   # destructuring compresses a multi-component X (LDLt.jl:54-57)
        BtLD = a * ((B.T @ L) @ Dm)
        EtL = np.asarray(E.T @ L)
        return L, Dm, BtLD, EtL, BtLD @ EtL.T          # K = (B'L D)(L'E)   (lowrank_ros1.jl:25-28)

    X = prob.X0
    Xs = [X]
    L, Dm, BtLD, EtL, K = feedback(X)
    Ks = [K]
    _call(observer, "observe_gdre_step", t[0], X, K)

    for i in range(1, nsteps + 1):
        tau = t[i - 1] - t[i]
        if order == 1:
            F = lr_update(ScaledPencil(A, 1.0, E, -1.0 / (2.0 * tau)), -1.0, B, K)                       # lowrank_ros1.jl:39
            G = np.hstack([Cm.T, EtL])
            S = np.zeros((G.shape[1],) * 2)
            S[:q, :q] = np.eye(q)
            S[q:, q:] = BtLD.T @ BtLD + Dm / tau                                                          # lowrank_ros1.jl:42-43
            rhs = compress_(lowrank(G, S))                                                                # :44
            X = step_solver(F)(rhs, X)                                                                    # :47-49 (warm start)
        else:
            # lr_update(A, alpha, U, V) = A + inv(alpha) U V (LowRankUpdate.jl:18-39): the reference passes inv(-gamma tau) for the term -gamma tau B K
            F = lr_update(ScaledPencil(A, gamma * tau, E, -0.5), 1.0 / (-gamma * tau), B, K)             # lowrank_ros2.jl:41
            lyap = step_solver(F)
            r = L.shape[1]
            G = np.hstack([Cm.T, np.asarray(A.T @ L), EtL])
            S = np.zeros((q + 2 * r,) * 2)
            S[:q, :q] = np.eye(q)
            S[q:q + r, q + r:] = Dm
            S[q + r:, q:q + r] = Dm
            S[q + r:, q + r:] = -(BtLD.T @ BtLD)                                                          # :44-55
            K1 = lyap(compress_(lowrank(G, S)), None)                                                     # :58
            a1, T1, D1 = K1
            BtT1D1 = a1 * ((B.T @ T1) @ D1)
            G2 = np.asarray(E.T @ T1)
            S2 = tau * tau * (BtT1D1.T @ BtT1D1) + (2.0 - 1.0 / gamma) * (a1 * D1)                        # :61-66
            K2 = lyap(lowrank(G2, S2), None)                                                              # :69
            X = X + ((2.0 - 1.0 / (2.0 * gamma)) * tau) * K1 + (-tau / 2.0) * K2                          # :72
        L, Dm, BtLD, EtL, K = feedback(X)
        Ks.append(K)
        if save_state:
            Xs.append(X)
        _call(observer, "observe_gdre_step", t[i], X, K)
    if not save_state:
        Xs.append(X)
    _call(observer, "observe_gdre_done")
    return DRESolution(Xs, Ks, t)


# ------------------------------------------------------------------------------------------------
# Factored sign-function solver (FactoredSign): LDLᵀ in, LDLᵀ out on a densified pencil           csrc/dense_sign_lr.hip
# in the place of solve(::GALEProblem{LDLᵀ}, ::ADI) (lyapunov/adi.jl) where no shifts can be found
# ------------------------------------------------------------------------------------------------
def _dense_operator(A):
    """A GALE coefficient (matrix, ScaledPencil, or a LowRankUpdate of either) as a dense Fortran-ordered matrix."""
    if isinstance(A, LowRankUpdate):
        return np.asfortranarray(_dense_operator(A.A) + (1.0 / A.alpha) * (np.asarray(A.U, float) @ np.asarray(A.V, float)))
    if isinstance(A, ScaledPencil):
        return np.asfortranarray(A.cA * _dense_f64(A.A) + A.cE * _dense_f64(A.E))
    return _dense_f64(A)


def _factored_sign_params(alg: FactoredSign, n):
    rtol = float(alg.rtol) if alg.rtol is not None else n * float(np.finfo(float).eps)
    return int(alg.maxiters), float(alg.tol) if alg.tol is not None else 0.0, rtol, int(alg.max_width), int(alg.max_refine)


class SignFactorization:
    """A kept sign iteration of one pencil (F, E) on the device (`dre_sign_create`): every further right-hand side costs a replay only.
    `E` and `F` are dense matrices (or anything `_dense_operator` densifies), or `DenseMatrix` objects already on the device."""

    def __init__(self, E, F, maxiters=50, tol=None, ctx=None):
        self.ctx = ctx or dev.default_context()
        Ed = E if isinstance(E, dev.DenseMatrix) else self.ctx.upload(_dense_operator(E))
        Fd = F if isinstance(F, dev.DenseMatrix) else self.ctx.upload(_dense_operator(F))
        self.n = Ed.shape[0]
        p = C.c_void_p()
        self.ctx.chk(self.ctx.lib.dre_sign_create(self.ctx.ptr, Ed.ptr, Fd.ptr, int(maxiters), float(tol) if tol is not None else 0.0, C.byref(p)))
        self.ptr = p
        self._fin = weakref.finalize(self, self.ctx.lib.dre_sign_free, self.ctx.ptr, p)
        it = C.c_int64()
        self.ctx.lib.dre_sign_info(p, C.byref(it))
        self.iters = int(it.value)

    def close(self):
        self._fin()

    def _entry(self, name, transposed):
        if not isinstance(transposed, (bool, np.bool_)):
            raise TypeError(f"transposed must be a bool, not {type(transposed).__name__}; nothing was run on the device")
        return getattr(self.ctx.lib, name + "_t" if transposed else name)

    def solve_lr(self, G, S, rtol=None, max_width=256, max_refine=1, download=True, *, transposed=False):
        """F'XE + E'XF = -G S G'  ->  (L, D, info) with X = L D L', D diagonal.  G, S: ndarrays or `DenseMatrix` objects on the device;
        download=False leaves L and D there (`DenseMatrix`).  transposed=True solves the dual equation F Y E' + E Y F' = -G S G' of the same
        pencil from the same kept factorisation (`dre_sign_solve_lr_t`)."""
        fn = self._entry("dre_sign_solve_lr", transposed)
        rtol = self.n * float(np.finfo(float).eps) if rtol is None else float(rtol)
        if isinstance(G, dev.DenseMatrix):
            Gd, Sd = G, S
        else:
            G = np.asarray(G, dtype=float).reshape(self.n, -1)
            r = G.shape[1]
            Gd, Sd = self.ctx.upload(G), self.ctx.upload(np.asarray(S, dtype=float).reshape(r, r))
        lp, dp = C.c_void_p(), C.c_void_p()
        ii, dd = (C.c_int64 * 4)(), (C.c_double * 2)()
        self.ctx.chk(fn(self.ctx.ptr, self.ptr, Gd.ptr, Sd.ptr, rtol, int(max_width), int(max_refine), C.byref(lp), C.byref(dp), ii, dd))
        L, Dm = dev.DenseMatrix(self.ctx, lp), dev.DenseMatrix(self.ctx, dp)
        if download:
            L, Dm = L.numpy(), Dm.numpy()
        return L, Dm, dict(iters=self.iters, rank=int(ii[0]), peak_width=int(ii[1]), compressions=int(ii[2]), refinements=int(ii[3]),
                           res0=float(dd[0]), res=float(dd[1]))

    def solve_dense(self, R, max_refine=2, download=True, *, transposed=False):
        """F'XE + E'XF = -R for a dense symmetric R (the `MatrixSign` replay on the kept factorisation) -> (X, info).  transposed=True solves
        the dual equation F Y E' + E Y F' = -R of the same pencil from the same kept factorisation (`dre_sign_solve_dense_t`)."""
        fn = self._entry("dre_sign_solve_dense", transposed)
        Rd = R if isinstance(R, dev.DenseMatrix) else self.ctx.upload(_dense_f64(R))
        xp = C.c_void_p()
        ii, dd = (C.c_int64 * 2)(), (C.c_double * 2)()
        self.ctx.chk(fn(self.ctx.ptr, self.ptr, Rd.ptr, int(max_refine), C.byref(xp), ii, dd))
        X = dev.DenseMatrix(self.ctx, xp)
        return (X.numpy() if download else X), dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1]))


def _single_block(Cl: LDLt):
    """(L, alpha D) of an LDLᵀ object, its components concatenated first"""
    if len(Cl.alphas) > 1:
        Cl = concatenate_(LDLt(list(Cl.alphas), list(Cl.Ls), list(Cl.Ds)))
    return np.asarray(Cl.Ls[0], float), Cl.alphas[0] * np.asarray(Cl.Ds[0], float)


def solve_gale_factored_sign(prob: GALEProblem, alg: FactoredSign, ctx=None, return_info=False, _sign=None):
    """solve(::GALEProblem{LDLᵀ}, ::FactoredSign) -> LDLᵀ: A'XE + E'XA = -C without shifts (in the place of lyapunov/adi.jl:3-147)."""
    if not isinstance(prob.C, LDLt):
        raise TypeError("FactoredSign() takes a low-rank right-hand side (an LDLᵀ object); a dense C (an ndarray) goes with MatrixSign()")
    n = prob.C.n
    maxiters, tol, rtol, max_width, max_refine = _factored_sign_params(alg, n)
    sign = _sign if _sign is not None else SignFactorization(prob.E, prob.A, maxiters, tol if tol > 0 else None, ctx)
    try:
        if prob.C.rank() == 0:
            G, S = np.zeros((n, 0)), np.zeros((0, 0))
        else:
            G, S = _single_block(prob.C)
        L, Dm, info = sign.solve_lr(G, S, rtol, max_width, max_refine)
    finally:
        if _sign is None:
            sign.close()
    X = lowrank(L, Dm)
    return (X, info) if return_info else X


def solve_gale_pair(E, A, C_obs, C_ctr, alg, ctx=None, return_info=False):
    """Both Lyapunov equations of one pencil from ONE sign factorisation (`dre_sign_create`) and two replays:
        A'XE + E'XA = -C_obs   (observability Gramian, regulator side)        A Y E' + E Y A' = -C_ctr   (controllability Gramian, filter side)
    -> (X, Y).  alg = MatrixSign(): the right-hand sides are ndarrays or LDLᵀ objects (densified), X and Y ndarrays; alg = FactoredSign(): both are
    LDLᵀ objects, and so are X and Y.  return_info=True adds dict(primal=..., dual=..., factorizations=1) with each replay's statistics."""
    if isinstance(alg, MatrixSign):
        for name, Cm in (("C_obs", C_obs), ("C_ctr", C_ctr)):
            if not isinstance(Cm, (LDLt, np.ndarray)) and not sp.issparse(Cm):
                raise TypeError(f"solve_gale_pair with MatrixSign() takes ndarray or LDLᵀ right-hand sides, {name} is a {type(Cm).__name__}; "
                                "nothing was run on the device")
    elif isinstance(alg, FactoredSign):
        for name, Cm in (("C_obs", C_obs), ("C_ctr", C_ctr)):
            if not isinstance(Cm, LDLt):
                raise TypeError(f"solve_gale_pair with FactoredSign() takes low-rank right-hand sides (LDLᵀ objects), {name} is a "
                                f"{type(Cm).__name__}; a dense right-hand side goes with MatrixSign(); nothing was run on the device")
    else:
        raise TypeError(f"solve_gale_pair takes alg = MatrixSign() or FactoredSign(), not {type(alg).__name__}; nothing was run on the device")
    if isinstance(alg, MatrixSign):
        maxiters, tol, max_refine = _sign_params(alg)
        Rs = [_dense_f64(Cm.dense() if isinstance(Cm, LDLt) else Cm) for Cm in (C_obs, C_ctr)]
        sign = SignFactorization(E, A, maxiters, tol if tol > 0 else None, ctx)
        try:
            X, ip = sign.solve_dense(Rs[0], max_refine)
            Y, idual = sign.solve_dense(Rs[1], max_refine, transposed=True)
        finally:
            sign.close()
    else:
        n = C_obs.n
        maxiters, tol, rtol, max_width, max_refine = _factored_sign_params(alg, n)
        blocks = [(np.zeros((n, 0)), np.zeros((0, 0))) if Cm.rank() == 0 else _single_block(Cm) for Cm in (C_obs, C_ctr)]
        sign = SignFactorization(E, A, maxiters, tol if tol > 0 else None, ctx)
        try:
            L, Dm, ip = sign.solve_lr(*blocks[0], rtol, max_width, max_refine)
            X = lowrank(L, Dm)
            L, Dm, idual = sign.solve_lr(*blocks[1], rtol, max_width, max_refine, transposed=True)
            Y = lowrank(L, Dm)
        finally:
            sign.close()
    return ((X, Y), dict(primal=ip, dual=idual, factorizations=1)) if return_info else (X, Y)


# ------------------------------------------------------------------------------------------------
# Device SVD and square-root balanced truncation                           csrc/svd_jacobi.hip, csrc/balance.hip
# ------------------------------------------------------------------------------------------------
def svd_jacobi(A, tol=None, ctx=None, return_stats=False):
    """svd(A) on the device by one-sided block Jacobi (`dre_svd_jacobi`): (U, s, V) with A ≈ U diag(s) Vᵀ, U m x k, s descending, V w x k,
    k = min(m, w).  Norm-wise accuracy (errors of order eps s[0]); no high relative accuracy for tiny singular values.  tol None:
    sqrt(max(m, w)) eps.  The columns of U (of V for a wide A) that belong to s <= tol ||A||_F are zero columns.  return_stats adds dict(sweeps, rounds, rank).
    A that is not a matrix and a tol that is not positive are errors before anything runs on the device; a non-finite entry is the device
    solver's DREError(-1)."""
    A = np.asarray(A, dtype=float)
    if A.ndim != 2:
        raise ValueError(f"svd_jacobi: a matrix is expected, got shape {A.shape}; nothing was run on the device")
    if tol is not None and not (float(tol) > 0.0 and math.isfinite(float(tol))):
        raise ValueError("svd_jacobi: tol must be positive and finite; nothing was run on the device")
    ctx = ctx or dev.default_context()
    Ad = ctx.upload(np.asfortranarray(A))
    up, sp_, vp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    ii = (C.c_int64 * 3)()
    ctx.chk(ctx.lib.dre_svd_jacobi(ctx.ptr, Ad.ptr, float(tol) if tol is not None else 0.0, C.byref(up), C.byref(sp_), C.byref(vp), ii))
    U, s, V = dev.DenseMatrix(ctx, up).numpy(), dev.DenseMatrix(ctx, sp_).numpy().ravel(), dev.DenseMatrix(ctx, vp).numpy()
    return (U, s, V, dict(sweeps=int(ii[0]), rounds=int(ii[1]), rank=int(ii[2]))) if return_stats else (U, s, V)


@dataclass
class ReducedModel:
    """ẋ_r = Ar x_r + Br u, y = Cr x_r (Er is the identity): the balanced truncation of E ẋ = A x + B u, y = C x to order len(Ar).  hsv: the
    Hankel singular values; T, W: the right and left projection (x ≈ T x_r, Wᵀ E T = I)."""
    Er: np.ndarray
    Ar: np.ndarray
    Br: np.ndarray
    Cr: np.ndarray
    hsv: np.ndarray
    T: np.ndarray
    W: np.ndarray

    @property
    def order(self):
        return self.Ar.shape[0]

    def freq_response(self, omega, D=None, **kw):
        """H_r(iω) = Cr (iω I - Ar)⁻¹ Br (+ D) of the reduced model at every frequency of omega, on the device: `freq_response` with E_r = I
        and its keyword arguments (method="embedding" | "complex" among them)."""
        return freq_response(self.Er, self.Ar, self.Br, self.Cr, omega, D=D, **kw)

    def step_response(self, dt, steps, D=None, **kw):
        """the step response of the reduced model on t_k = k dt, (steps + 1, q, m), on the device: `step_response` with E_r = I and its keywords"""
        return step_response(self.Er, self.Ar, self.Br, self.Cr, dt, steps, D=D, **kw)

    def impulse_response(self, dt, steps, **kw):
        """the impulse response of the reduced model, (steps + 1, q, m), on the device: `impulse_response` with E_r = I and its keywords"""
        return impulse_response(self.Er, self.Ar, self.Br, self.Cr, dt, steps, **kw)

    def simulate(self, u, dt, x0=None, D=None, **kw):
        """the reduced model's output for the input samples u (x0 in reduced coordinates), on the device: `simulate` with E_r = I and its keywords"""
        return simulate(self.Er, self.Ar, self.Br, self.Cr, u, dt, x0=x0, D=D, **kw)


def _balance_check(name, E, A, B, C, alg, order, tol):
    if not isinstance(alg, (FactoredSign, MatrixSign)):
        raise TypeError(f"{name} takes alg = FactoredSign() or MatrixSign(), not {type(alg).__name__}; nothing was run on the device")
    if order is not None and (isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer))):
        raise TypeError(f"{name}: order must be None or an int, not {type(order).__name__}; nothing was run on the device")
    if order is not None and order < 1:
        raise ValueError(f"{name}: order must be at least 1 (None: chosen by tol); nothing was run on the device")
    if not (isinstance(tol, (int, float, np.floating)) and math.isfinite(tol) and tol >= 0.0):
        raise ValueError(f"{name}: tol must be a finite non-negative number; nothing was run on the device")
    mats = []
    for nm, M in (("E", E), ("A", A), ("B", B), ("C", C)):
        if not isinstance(M, (np.ndarray, LowRankUpdate, ScaledPencil)) and not sp.issparse(M):
            raise TypeError(f"{name}: {nm} must be a matrix, not {type(M).__name__}; nothing was run on the device")
        mats.append(_dense_operator(M))
    Ed, Am, Bm, Cm = mats
    n = Ed.shape[0]
    if Ed.ndim != 2 or Ed.shape != (n, n) or Am.shape != (n, n) or Bm.ndim != 2 or Bm.shape[0] != n or Cm.ndim != 2 or Cm.shape[1] != n:
        raise ValueError(f"{name}: E and A must be n x n, B n x m and C q x n; got {Ed.shape}, {Am.shape}, {Bm.shape}, {Cm.shape}; "
                         "nothing was run on the device")
    return Ed, Am, Bm, Cm


def _balance(name, E, A, B, Cout, alg, order, tol, ctx):
    Eh, Ah, Bh, Ch = _balance_check(name, E, A, B, Cout, alg, order, tol)
    n = Eh.shape[0]
    ctx = ctx or dev.default_context()
    Ed, Ad, Bd, Cd = (ctx.upload(M) for M in (Eh, Ah, Bh, Ch))
    if isinstance(alg, FactoredSign):
        maxiters, stol, rtol, max_width, max_refine = _factored_sign_params(alg, n)
    else:
        maxiters, stol, max_refine = _sign_params(alg)
    sign = SignFactorization(Ed, Ad, maxiters, stol if stol > 0 else None, ctx)
    try:
        if isinstance(alg, FactoredSign):
            Lo, Do, ip = sign.solve_lr(ctx.upload(np.asfortranarray(Ch.T)), ctx.upload(np.eye(Ch.shape[0])), rtol, max_width, max_refine, download=False)
            Lc, Dc, idual = sign.solve_lr(Bd, ctx.upload(np.eye(Bh.shape[1])), rtol, max_width, max_refine, download=False, transposed=True)
        else:
            Q, ip = sign.solve_dense(ctx.gemm(True, False, 1.0, Cd, Cd), max_refine, download=False)
            P, idual = sign.solve_dense(ctx.gemm(False, True, 1.0, Bd, Bd), max_refine, download=False, transposed=True)
            fac = []
            for X in (Q, P):
                wp, vp = C.c_void_p(), C.c_void_p()
                ctx.chk(ctx.lib.dre_sym_eig(ctx.ptr, X.ptr, 4.0, C.byref(wp), C.byref(vp)))
                fac.append((dev.DenseMatrix(ctx, vp), dev.DenseMatrix(ctx, wp)))
            (Lo, Do), (Lc, Dc) = fac
    finally:
        sign.close()
    out = [C.c_void_p() for _ in range(6)]
    ii, dd = (C.c_int64 * 6)(), (C.c_double * 3)()
    ctx.chk(ctx.lib.dre_balance_lr(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, Cd.ptr, Lc.ptr, Dc.ptr, Lo.ptr, Do.ptr, int(order or 0), float(tol),
                                   *(C.byref(p) for p in out), ii, dd))
    hsv, T, W, Ar, Br, Cr = (dev.DenseMatrix(ctx, p).numpy() for p in out)
    info = dict(primal=ip, dual=idual, factorizations=1, order=int(ii[0]), rank=int(ii[1]), r_c=int(ii[2]), r_o=int(ii[3]), dropped=int(ii[4]),
                svd_sweeps=int(ii[5]), eye_err=float(dd[0]), bound=float(dd[1]), neg_max=float(dd[2]))
    return ReducedModel(np.eye(Ar.shape[0]), Ar, Br, Cr, hsv.ravel(), T, W), info


def balanced_truncation(E, A, B, C, alg=FactoredSign(), order=None, tol=1e-8, ctx=None, return_info=False):
    """Square-root balanced truncation of E ẋ = A x + B u, y = C x (c-stable pencil (A, E)) on the device -> ReducedModel.
    ONE sign factorisation of (A, E) (`dre_sign_create`) and two replays give the Gramians: alg = FactoredSign() keeps them in factored form on
    the device, alg = MatrixSign() runs the two dense replays and factors each Gramian with `dre_sym_eig`.  `dre_balance_lr` does the rest: the
    SVD of Z_oᵀ E Z_c by `dre_svd_jacobi`, the order, the projections and the reduced matrices.
    order: the reduced order (above the numerical rank of Z_oᵀ E Z_c: DREError(-1)); None: the smallest r with 2 Σ_{i>r} σ_i <= tol σ_1.
    return_info=True adds dict(primal, dual, factorizations=1, order, rank, r_c, r_o, dropped, svd_sweeps, eye_err = ||WᵀET - I||_F,
    bound = 2 Σ_{i>r} σ_i, neg_max).  Wrong types and shapes are errors before anything runs on the device."""
    red, info = _balance("balanced_truncation", E, A, B, C, alg, order, tol, ctx)
    return (red, info) if return_info else red


def hankel_singular_values(E, A, B, C, alg=FactoredSign(), ctx=None):
    """The Hankel singular values of E ẋ = A x + B u, y = C x, descending (the `hsv` of `balanced_truncation`)."""
    return _balance("hankel_singular_values", E, A, B, C, alg, None, 0.0, ctx)[0].hsv


# ------------------------------------------------------------------------------------------------
# Ensembles: batched block Jacobi and ensemble balanced truncation          csrc/sym_jacobi.hip, csrc/svd_jacobi.hip, csrc/balance.hip
# ------------------------------------------------------------------------------------------------
def _batch_members(name, As, what="matrices"):
    if isinstance(As, np.ndarray) and As.ndim == 3:
        As = list(As)
    if not isinstance(As, (list, tuple)):
        raise TypeError(f"{name}: a list of {what} is expected, not {type(As).__name__}; nothing was run on the device")
    if len(As) == 0:
        raise ValueError(f"{name}: empty list of {what}; nothing was run on the device")
    if len(As) > 65535:
        raise ValueError(f"{name}: a batch has at most 65535 members, got {len(As)}; nothing was run on the device")
    return list(As)


def _batch_errors_arg(name, errors):
    if errors not in ("raise", "return"):
        raise ValueError(f'{name}: errors must be "raise" or "return"; nothing was run on the device')


def _raise_first(out, errors):
    if errors == "raise":
        for e in out:
            if isinstance(e, DREError):
                raise e
    return out


def sym_eigh_batch(As, tol=None, errors="raise", ctx=None, return_stats=False):
    """eigh(A_b) of a list of dense symmetric matrices of one order in shared launches (`dre_sym_eig_jacobi_batched`, the block Jacobi solver of
    sym_eigh(method="jacobi") with the member on a grid axis): the list of (w, V), w ascending; with return_stats (w, V, dict(sweeps, rounds)).
    Every member's result is bit for bit what sym_eigh returns for it alone.  A member with a non-finite entry fails alone (DREError(-1));
    errors="raise" raises the first failed member's error, errors="return" puts the DREError in that member's slot.  The shape and symmetry
    checks of sym_eigh are made for every member before anything runs on the device."""
    name = "sym_eigh_batch"
    As = [np.asarray(A, dtype=float) for A in _batch_members(name, As)]
    _batch_errors_arg(name, errors)
    if tol is not None and not float(tol) > 0.0:
        raise ValueError(f"{name}: tol must be positive; nothing was run on the device")
    for b, A in enumerate(As):
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError(f"{name}: member {b}: a square matrix is expected, got shape {A.shape}; nothing was run on the device")
        if A.shape != As[0].shape:
            raise ValueError(f"{name}: member {b} has shape {A.shape}, member 0 has {As[0].shape}: the members of a batch share one order; "
                             "nothing was run on the device")
        if A.size and np.isfinite(A).all():           # (a non-finite entry is the device solver's DRE_ERR_INVALID of that member)
            asym = np.abs(A - A.T).max()
            if asym > 100 * np.finfo(float).eps * np.abs(A).max():
                raise ValueError(f"{name}: member {b} is not symmetric (max |A - A'| = {asym:.3e}); nothing was run on the device")
    nb, n = len(As), As[0].shape[0]
    if n == 0:
        return [(np.zeros(0), np.zeros((0, 0)), dict(sweeps=0, rounds=0)) if return_stats else (np.zeros(0), np.zeros((0, 0))) for _ in As]
    ctx = ctx or dev.default_context()
    Ad = [ctx.upload(np.asfortranarray(A)) for A in As]
    ws, vs = (C.c_void_p * nb)(), (C.c_void_p * nb)()
    ii, status = np.zeros(2 * nb, dtype=np.int64), np.zeros(nb, dtype=np.int32)
    ctx.chk(ctx.lib.dre_sym_eig_jacobi_batched(ctx.ptr, nb, _handle_array(Ad), float(tol) if tol is not None else 0.0, ws, vs,
                                               ii.ctypes.data_as(C.POINTER(C.c_int64)), status.ctypes.data_as(C.POINTER(C.c_int32))))
    errs = _batch_errors(ctx, status)
    out = []
    for b in range(nb):
        if errs[b] is not None:
            out.append(errs[b])
            continue
        w, V = dev.DenseMatrix(ctx, C.c_void_p(ws[b])).numpy().ravel(), dev.DenseMatrix(ctx, C.c_void_p(vs[b])).numpy()
        out.append((w, V, dict(sweeps=int(ii[2 * b]), rounds=int(ii[2 * b + 1]))) if return_stats else (w, V))
    return _raise_first(out, errors)


def svd_jacobi_batch(As, tol=None, errors="raise", ctx=None, return_stats=False):
    """svd(A_b) of a list of matrices of one shape in shared launches (`dre_svd_jacobi_batched`, the one-sided block Jacobi of svd_jacobi with
    the member on a grid axis): the list of (U, s, V); with return_stats (U, s, V, dict(sweeps, rounds, rank)).  Every member's result is bit
    for bit what svd_jacobi returns for it alone.  A member with a non-finite entry fails alone (DREError(-1)); errors as in sym_eigh_batch.
    A member that is not a matrix, two shapes in one batch and a tol that is not positive are errors before anything runs on the device."""
    name = "svd_jacobi_batch"
    As = [np.asarray(A, dtype=float) for A in _batch_members(name, As)]
    _batch_errors_arg(name, errors)
    if tol is not None and not (float(tol) > 0.0 and math.isfinite(float(tol))):
        raise ValueError(f"{name}: tol must be positive and finite; nothing was run on the device")
    for b, A in enumerate(As):
        if A.ndim != 2:
            raise ValueError(f"{name}: member {b}: a matrix is expected, got shape {A.shape}; nothing was run on the device")
        if A.shape != As[0].shape:
            raise ValueError(f"{name}: member {b} has shape {A.shape}, member 0 has {As[0].shape}: the members of a batch share one shape; "
                             "nothing was run on the device")
    nb = len(As)
    ctx = ctx or dev.default_context()
    Ad = [ctx.upload(np.asfortranarray(A)) for A in As]
    us, ss, vs = (C.c_void_p * nb)(), (C.c_void_p * nb)(), (C.c_void_p * nb)()
    ii, status = np.zeros(3 * nb, dtype=np.int64), np.zeros(nb, dtype=np.int32)
    ctx.chk(ctx.lib.dre_svd_jacobi_batched(ctx.ptr, nb, _handle_array(Ad), float(tol) if tol is not None else 0.0, us, ss, vs,
                                           ii.ctypes.data_as(C.POINTER(C.c_int64)), status.ctypes.data_as(C.POINTER(C.c_int32))))
    errs = _batch_errors(ctx, status)
    out = []
    for b in range(nb):
        if errs[b] is not None:
            out.append(errs[b])
            continue
        U, s, V = (dev.DenseMatrix(ctx, C.c_void_p(h[b])).numpy() for h in (us, ss, vs))
        st = dict(sweeps=int(ii[3 * b]), rounds=int(ii[3 * b + 1]), rank=int(ii[3 * b + 2]))
        out.append((U, s.ravel(), V, st) if return_stats else (U, s.ravel(), V))
    return _raise_first(out, errors)


BALANCE_BATCH_MAX_N = 4096      # the batched dense Lyapunov solver's order limit (dre_dense_gale_solve_batched)


def _balance_batch_check(systems, alg, order, tol, errors):
    name = "balanced_truncation_batch"
    systems = _batch_members(name, systems, "(E, A, B, C) systems")
    _batch_errors_arg(name, errors)
    if isinstance(alg, FactoredSign):
        raise TypeError(f"{name}: the batched route is the dense one, alg = MatrixSign(); FactoredSign() Gramians are not batched "
                        "(balanced_truncation takes them one system at a time); nothing was run on the device")
    if not isinstance(alg, MatrixSign):
        raise TypeError(f"{name} takes alg = MatrixSign(), not {type(alg).__name__}; nothing was run on the device")
    mats = []
    for b, sys_ in enumerate(systems):
        if not isinstance(sys_, (tuple, list)) or len(sys_) != 4:
            raise TypeError(f"{name}: member {b} must be a tuple (E, A, B, C); nothing was run on the device")
        mats.append(_balance_check(f"{name}: member {b}", *sys_, alg, order, tol))
    shape = lambda m: (m[0].shape[0], m[2].shape[1], m[3].shape[0])
    for b, m in enumerate(mats):
        if shape(m) != shape(mats[0]):
            raise ValueError(f"{name}: member {b} has (n, m, q) = {shape(m)}, member 0 has {shape(mats[0])}: the members of a batch share n, m "
                             "and q; nothing was run on the device")
    n = shape(mats[0])[0]
    if not 1 <= n <= BALANCE_BATCH_MAX_N:
        raise ValueError(f"{name}: the batched dense Lyapunov solver takes orders 1 .. {BALANCE_BATCH_MAX_N}, got n = {n}; nothing was run on the device")
    if 2 * len(mats) > 65535:
        raise ValueError(f"{name}: at most 32767 systems (two Lyapunov equations each in one batch), got {len(mats)}; nothing was run on the device")
    return mats


def balanced_truncation_batch(systems, alg=MatrixSign(), order=None, tol=1e-8, errors="raise", ctx=None, return_info=False):
    """Square-root balanced truncation of an ensemble: a list of (E, A, B, C) of one (n, m, q), n <= 4096 -> the list of ReducedModel, in three
    batched calls:  (1) ONE `dre_dense_gale_solve_batched` of 2B members gives both Gramians of every system (member b: A'QE + E'QA = -C'C, member
    B + b: the transposed pencil, A P E' + E P A' = -B B');  (2) ONE `dre_sym_eig_jacobi_batched` factors the 2B Gramians, and eigenvalues at or
    below n eps lambda_max are set to zero;  (3) ONE `dre_balance_lr_batched`: every Z_o'E Z_c in a zero-padded stack of the common shape
    (max r_o) x (max r_c), one batched SVD, then the order rule, projections and reduced matrices per member.
    A member's result is a bitwise function of its own data and of the padded shape only.  A member whose pencil is not c-stable
    (DREError(-7)), or whose `order` is above its numerical rank (DREError(-1)), fails alone: errors="raise" raises the first failed member's
    error, errors="return" puts the DREError in its slot.  return_info=True gives (ReducedModel, info) per member, info with the keys of
    balanced_truncation's (primal, dual: the two Lyapunov solves; factorizations = 2, one per Gramian) plus padded_shape.
    FactoredSign() is a TypeError (the batched route is the dense one); wrong types and shapes are errors before anything runs on the device."""
    mats = _balance_batch_check(systems, alg, order, tol, errors)
    nb, n = len(mats), mats[0][0].shape[0]
    ctx = ctx or dev.default_context()
    lib = ctx.lib
    pi32, pi64, pd = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    ups = [[ctx.upload(M) for M in m] for m in mats]                                    # (E, A, B, C) handles per member
    # (1) the Gramians: members 0 .. B-1 (E, A, C'C), members B .. 2B-1 (E', A', B B')
    maxiters, stol, max_refine = _sign_params(alg)
    Es = [u[0] for u in ups] + [ctx.upload(np.asfortranarray(m[0].T)) for m in mats]
    Fs = [u[1] for u in ups] + [ctx.upload(np.asfortranarray(m[1].T)) for m in mats]
    Rs = [ctx.gemm(True, False, 1.0, u[3], u[3]) for u in ups] + [ctx.gemm(False, True, 1.0, u[2], u[2]) for u in ups]
    xs = (C.c_void_p * (2 * nb))()
    gi, gd, gst = np.zeros(4 * nb, dtype=np.int64), np.zeros(4 * nb), np.zeros(2 * nb, dtype=np.int32)
    ctx.chk(lib.dre_dense_gale_solve_batched(ctx.ptr, 2 * nb, _handle_array(Es), _handle_array(Fs), _handle_array(Rs), maxiters, stol, max_refine, xs,
                                             gi.ctypes.data_as(pi64), gd.ctypes.data_as(pd), gst.ctypes.data_as(pi32)))
    def member_error(b, e, stage):
        """a batched call's error of one of its members, renumbered to the system it belongs to"""
        msg = str(e).split(": ", 1)[1] if ": " in str(e) else str(e)
        return DREError(e.code, f"balanced_truncation_batch, member {b} ({stage}): {msg}")

    gerr = _batch_errors(ctx, gst)
    X = [dev.DenseMatrix(ctx, C.c_void_p(xs[j])) if gerr[j] is None else None for j in range(2 * nb)]
    gstat = [dict(iters=int(gi[2 * j]), refinements=int(gi[2 * j + 1]), res0=float(gd[2 * j]), res=float(gd[2 * j + 1])) for j in range(2 * nb)]
    out = [None] * nb                                                                   # None: still alive
    for b in range(nb):
        for j, stage in ((b, "observability Gramian"), (nb + b, "controllability Gramian")):
            if gerr[j] is not None and out[b] is None:
                out[b] = member_error(b, gerr[j], stage)
    del Es, Fs, Rs

    def alive():
        return [b for b in range(nb) if out[b] is None]

    # (2) the eigen-decompositions of the Gramians of the members still alive: Q_b then P_b
    live = alive()
    fac = {}
    if live:
        G = [X[b] for b in live] + [X[nb + b] for b in live]
        k = len(G)
        ws, vs = (C.c_void_p * k)(), (C.c_void_p * k)()
        est = np.zeros(k, dtype=np.int32)
        ctx.chk(lib.dre_sym_eig_jacobi_batched(ctx.ptr, k, _handle_array(G), 0.0, ws, vs, None, est.ctypes.data_as(pi32)))
        eerr = _batch_errors(ctx, est)
        for i, b in enumerate(live):
            for j, stage in ((i, "observability Gramian's eigen-decomposition"), (len(live) + i, "controllability Gramian's eigen-decomposition")):
                if eerr[j] is not None and out[b] is None:
                    out[b] = member_error(b, eerr[j], stage)
        for i, b in enumerate(live):
            pair = []
            for j in (i, len(live) + i):                                                # observability, controllability
                if eerr[j] is not None:
                    continue
                w, V = dev.DenseMatrix(ctx, C.c_void_p(ws[j])), dev.DenseMatrix(ctx, C.c_void_p(vs[j]))
                lam = w.numpy().ravel()
                lam[lam <= n * np.finfo(float).eps * lam.max()] = 0.0                   # the reference's rule (tests/_balance_cases.py, rank_rtol)
                pair.append((V, ctx.upload(lam.reshape(-1, 1)), int((lam > 0).sum())))
            if out[b] is None:
                fac[b] = pair
    del X

    # (3) the SVD of the stack and the reduced models
    live = alive()
    res = {}
    if live:
        k = len(live)
        padded = (max(fac[b][0][2] for b in live), max(fac[b][1][2] for b in live))
        arrs = [_handle_array([ups[b][j] for b in live]) for j in range(4)]
        arrs += [_handle_array([fac[b][1][0] for b in live]), _handle_array([fac[b][1][1] for b in live]),
                 _handle_array([fac[b][0][0] for b in live]), _handle_array([fac[b][0][1] for b in live])]
        outs = [(C.c_void_p * k)() for _ in range(6)]
        ii, dd, bst = np.zeros(6 * k, dtype=np.int64), np.zeros(3 * k), np.zeros(k, dtype=np.int32)
        ctx.chk(lib.dre_balance_lr_batched(ctx.ptr, k, *arrs, int(order or 0), float(tol), *outs, ii.ctypes.data_as(pi64), dd.ctypes.data_as(pd),
                                           bst.ctypes.data_as(pi32)))
        berr = _batch_errors(ctx, bst)
        for i, b in enumerate(live):
            if berr[i] is not None:
                out[b] = member_error(b, berr[i], "balancing")
                continue
            hsv, T, W, Ar, Br, Cr = (dev.DenseMatrix(ctx, C.c_void_p(o[i])).numpy() for o in outs)
            j, d = ii[6 * i:6 * i + 6], dd[3 * i:3 * i + 3]
            info = dict(primal=gstat[b], dual=gstat[nb + b], factorizations=2, order=int(j[0]), rank=int(j[1]), r_c=int(j[2]), r_o=int(j[3]),
                        dropped=int(j[4]), svd_sweeps=int(j[5]), eye_err=float(d[0]), bound=float(d[1]), neg_max=float(d[2]), padded_shape=padded)
            red = ReducedModel(np.eye(Ar.shape[0]), Ar, Br, Cr, hsv.ravel(), T, W)
            res[b] = (red, info) if return_info else red
    for b in range(nb):
        if out[b] is None:
            out[b] = res[b]
    return _raise_first(out, errors)


# ------------------------------------------------------------------------------------------------
# Frequency response, batched by frequency                                  csrc/freq_response.hip
# ------------------------------------------------------------------------------------------------
FREQ_RESPONSE_MAX_N = 2048      # the real form of iωE - A has order 2n and is inverted with the register panel (2n <= 4096)
TRANSFER_MAX_N = COMPLEX_PANEL_MAX_N   # method="complex": s E - A itself goes through the complex register panel
FREQ_METHODS = ("embedding", "complex")


def _freq_method(name, method):
    if method not in FREQ_METHODS:
        raise ValueError(f"{name}: method must be 'embedding' (the real form of order 2n, n <= {FREQ_RESPONSE_MAX_N}) or 'complex' (the complex "
                         f"Gauss-Jordan inversion, n <= {TRANSFER_MAX_N}), got {method!r}; nothing was run on the device")


def _freq_check(name, systems, omega, D, errors, chunk, method="embedding", points=False):
    """the argument errors of the frequency-response calls, before anything runs on the device -> (list of (E, A, B, C), omega, D); points:
    omega holds complex points s (transfer_function), not real frequencies"""
    _batch_errors_arg(name, errors)
    _freq_method(name, method)
    if chunk is not None and (isinstance(chunk, (bool, np.bool_)) or not isinstance(chunk, (int, np.integer)) or not 1 <= chunk <= 65535):
        raise ValueError(f"{name}: chunk must be None (as many frequencies as fit) or an int in 1 .. 65535; nothing was run on the device")
    what = "s" if points else "omega"
    w = np.asarray(omega, dtype=complex if points else float)
    if w.ndim != 1:
        raise ValueError(f"{name}: {what} must be a one-dimensional array of {'points' if points else 'frequencies'}, got shape {w.shape}; nothing "
                         "was run on the device")
    if w.size < 1:
        raise ValueError(f"{name}: at least one {'point' if points else 'frequency'} is needed; nothing was run on the device")
    if not np.isfinite(w).all():
        raise ValueError(f"{name}: {what} has a non-finite entry; nothing was run on the device")
    mats = []
    for b, sys_ in enumerate(systems):
        ms = []
        for nm, M in zip("EABC", sys_):
            if not isinstance(M, (np.ndarray, LowRankUpdate, ScaledPencil)) and not sp.issparse(M):
                raise TypeError(f"{name}: {nm} must be a matrix, not {type(M).__name__}; nothing was run on the device")
            ms.append(_dense_f64(_dense_operator(M)))
        Ed, Am, Bm, Cm = ms
        n = Ed.shape[0]
        if Ed.ndim != 2 or Ed.shape != (n, n) or Am.shape != (n, n) or Bm.ndim != 2 or Bm.shape[0] != n or Cm.ndim != 2 or Cm.shape[1] != n \
                or n < 1 or Bm.shape[1] < 1 or Cm.shape[0] < 1:
            raise ValueError(f"{name}: E and A must be n x n, B n x m and C q x n (n, m, q >= 1); got {Ed.shape}, {Am.shape}, {Bm.shape}, {Cm.shape}; "
                             "nothing was run on the device")
        mats.append((Ed, Am, Bm, Cm))
    shape = lambda t: (t[0].shape[0], t[2].shape[1], t[3].shape[0])
    for b, t in enumerate(mats):
        if shape(t) != shape(mats[0]):
            raise ValueError(f"{name}: member {b} has (n, m, q) = {shape(t)}, member 0 has {shape(mats[0])}: the systems of a batch share n, m "
                             "and q; nothing was run on the device")
    n, m, q = shape(mats[0])
    if method == "embedding" and n > FREQ_RESPONSE_MAX_N:
        raise ValueError(f"{name}: the real form of i omega E - A has order 2n and goes through the register panel, n <= {FREQ_RESPONSE_MAX_N}; "
                         f"got n = {n}; nothing was run on the device")
    if method == "complex" and n > TRANSFER_MAX_N:
        raise ValueError(f"{name}: s E - A goes through the complex register panel, n <= {TRANSFER_MAX_N}; got n = {n}; nothing was run on the "
                         "device")
    if D is not None:
        D = np.asarray(D)
        if D.shape != (q, m):
            raise ValueError(f"{name}: D must be q x m = {(q, m)}, got {D.shape}; nothing was run on the device")
    return mats, w, D


def _freq_run(name, mats, w, chunk, ctx, method="embedding"):
    """-> (H (nsys, K, q, m) complex, list of DREError / None per member s K + k, info).  method="embedding": w real frequencies
    (`dre_freq_response`); "complex": w complex points (`dre_transfer_eval`)"""
    ctx = ctx or dev.default_context()
    nsys, K = len(mats), w.size
    n, m, q = mats[0][0].shape[0], mats[0][2].shape[1], mats[0][3].shape[0]
    ups = [[ctx.upload(M) for M in t] for t in mats]
    re, im = np.zeros(nsys * K * q * m), np.zeros(nsys * K * q * m)
    status, info = np.zeros(nsys * K, dtype=np.int32), (C.c_int64 * 2)()
    pd, pi32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    if method == "complex":
        pts = np.asarray(w, dtype=complex)
        sr, si = np.ascontiguousarray(pts.real), np.ascontiguousarray(pts.imag)
        points, single, batched = (sr.ctypes.data_as(pd), si.ctypes.data_as(pd)), ctx.lib.dre_transfer_eval, ctx.lib.dre_transfer_eval_batched
    else:
        wc = np.ascontiguousarray(w)
        points, single, batched = (wc.ctypes.data_as(pd),), ctx.lib.dre_freq_response, ctx.lib.dre_freq_response_batched
    tail = (K, *points, int(chunk or 0), re.ctypes.data_as(pd), im.ctypes.data_as(pd), status.ctypes.data_as(pi32), info)
    if nsys == 1:
        ctx.chk(single(ctx.ptr, *(u.ptr for u in ups[0]), *tail))
    else:
        ctx.chk(batched(ctx.ptr, nsys, *(_handle_array([u[j] for u in ups]) for j in range(4)), *tail))
    H = (re + 1j * im).reshape(nsys, K, m, q).transpose(0, 1, 3, 2)         # members hold q x m column-major
    return H, _batch_errors(ctx, status), dict(chunk=int(info[0]), chunks=int(info[1]), members=nsys * K, order=n if method == "complex" else 2 * n)


def _freq_out(H, errs, info, errors, return_info):
    if errors == "raise":
        _raise_first(errs, errors)
        return (H, info) if return_info else H
    return (H, errs, info) if return_info else (H, errs)


def _freq_points(w, method):
    """what _freq_run takes: the frequencies themselves, or the points i w of the complex method"""
    return 1j * w if method == "complex" else w


def freq_response(E, A, B, C, omega, D=None, errors="raise", chunk=None, ctx=None, return_info=False, method="embedding"):
    """H(iω_k) = C (iω_k E - A)⁻¹ B + D of the dense descriptor system E ẋ = A x + B u, y = C x + D u at every frequency of omega, in shared
    launches with the frequency on the member axis: a complex array (K, q, m).
    method="embedding" (the default, `dre_freq_response`): per frequency the real form [[-A, -ωE], [ωE, -A]] of iωE - A is inverted with the
    register panel, so n <= 2048; 16 n³ flops and 4 n² doubles per frequency.  method="complex" (`dre_transfer_eval` at s = iω): iωE - A
    itself is inverted by the complex Gauss-Jordan panel, n <= 4096; 8 n³ flops and 2 n² doubles per frequency; the two agree to rounding,
    not bit for bit.  E may be singular; D (q x m) is added on the host.  The sweep runs in chunks of `chunk` frequencies (None: as many as
    fit the device memory); a frequency's result is bit for bit the same whatever the others are and whatever chunk it falls in.
    A frequency at which iωE - A is exactly singular (ω on a pole, a NaN in the system) fails alone: its H is NaN.  errors="raise" raises that
    DREError(-4); errors="return" returns (H, errs) with errs[k] None or the DREError of frequency k.  return_info=True appends
    dict(chunk, chunks, members, order = 2n, or n for "complex").  Wrong types, shapes, an unknown method, a non-finite ω and an empty omega
    are errors before anything runs on the device."""
    name = "freq_response"
    mats, w, D = _freq_check(name, [(E, A, B, C)], omega, D, errors, chunk, method)
    H, errs, info = _freq_run(name, mats, _freq_points(w, method), chunk, ctx, method)
    H = H[0] if D is None else H[0] + D
    return _freq_out(H, errs, info, errors, return_info)


def freq_response_batch(systems, omega, errors="raise", chunk=None, ctx=None, return_info=False, method="embedding"):
    """`freq_response` for an ensemble: systems is the list of (E, A, B, C) of one (n, m, q) that `balanced_truncation_batch` takes -> a
    complex array (nsys, K, q, m) from one `dre_freq_response_batched` call (method="complex": one `dre_transfer_eval_batched` call, n <=
    4096), member s K + k = system s at ω_k.  Entry (s, k) is bit for bit what freq_response gives for system s at ω_k with the same
    method.  errors="return": (H, errs) with errs[s][k]."""
    name = "freq_response_batch"
    systems = _batch_members(name, systems, "(E, A, B, C) systems")
    for b, sys_ in enumerate(systems):
        if not isinstance(sys_, (tuple, list)) or len(sys_) != 4:
            raise TypeError(f"{name}: member {b} must be a tuple (E, A, B, C); nothing was run on the device")
    mats, w, _ = _freq_check(name, systems, omega, None, errors, chunk, method)
    H, errs, info = _freq_run(name, mats, _freq_points(w, method), chunk, ctx, method)
    if errors == "raise":
        return _freq_out(H, errs, info, errors, return_info)
    K = w.size
    return _freq_out(H, [errs[s * K:(s + 1) * K] for s in range(len(mats))], info, errors, return_info)


def transfer_function(E, A, B, C, s, D=None, errors="raise", chunk=None, ctx=None, return_info=False):
    """H(s_k) = C (s_k E - A)⁻¹ B + D at every complex point of s, in shared launches with the point on the member axis
    (`dre_transfer_eval`): a complex array (K, q, m).  Per point the planes of s E - A are inverted by the complex Gauss-Jordan panel
    (n <= 4096; 8 n³ flops, 2 n² doubles), with one refinement step whose residual is formed from E and A.  Points off the imaginary axis
    are what interpolation-based model reduction and pole/zero work need; at s = iω this is `freq_response(..., method="complex")`.
    Everything else is `freq_response`'s: E may be singular, D is added on the host, chunks, a point on a pole fails alone (DREError(-4), its
    H NaN), errors="return", return_info (order = n), and the argument errors before anything runs on the device (a non-finite point among
    them)."""
    name = "transfer_function"
    mats, pts, D = _freq_check(name, [(E, A, B, C)], s, D, errors, chunk, "complex", points=True)
    H, errs, info = _freq_run(name, mats, pts, chunk, ctx, "complex")
    H = H[0] if D is None else H[0] + D
    return _freq_out(H, errs, info, errors, return_info)


def transfer_function_batch(systems, s, errors="raise", chunk=None, ctx=None, return_info=False):
    """`transfer_function` for an ensemble of (E, A, B, C) of one (n, m, q) -> a complex array (nsys, K, q, m) from one
    `dre_transfer_eval_batched` call, member s K + k = system s at point k, bit for bit what transfer_function gives for it.
    errors="return": (H, errs) with errs[s][k]."""
    name = "transfer_function_batch"
    systems = _batch_members(name, systems, "(E, A, B, C) systems")
    for b, sys_ in enumerate(systems):
        if not isinstance(sys_, (tuple, list)) or len(sys_) != 4:
            raise TypeError(f"{name}: member {b} must be a tuple (E, A, B, C); nothing was run on the device")
    mats, pts, _ = _freq_check(name, systems, s, None, errors, chunk, "complex", points=True)
    H, errs, info = _freq_run(name, mats, pts, chunk, ctx, "complex")
    if errors == "raise":
        return _freq_out(H, errs, info, errors, return_info)
    K = pts.size
    return _freq_out(H, [errs[i * K:(i + 1) * K] for i in range(len(mats))], info, errors, return_info)


def sigma_response(E, A, B, C, omega, D=None, errors="raise", chunk=None, ctx=None, return_info=False, method="embedding"):
    """The singular values of H(iω_k), descending: a real array (K, min(q, m)), the data of a sigma plot.  H comes from `freq_response` (same
    arguments and returns, `method` among them); the K tiny SVDs run on the host on purpose (numpy.linalg.svd).  A failed frequency's row
    is NaN."""
    out = freq_response(E, A, B, C, omega, D=D, errors=errors, chunk=chunk, ctx=ctx, return_info=return_info, method=method)
    H = out[0] if isinstance(out, tuple) else out
    S = np.full((H.shape[0], min(H.shape[1:])), np.nan)
    ok = np.isfinite(H).all(axis=(1, 2))
    if ok.any():
        S[ok] = np.linalg.svd(H[ok], compute_uv=False)
    return (S,) + out[1:] if isinstance(out, tuple) else S


def bt_error(E, A, B, C, rom, omega, chunk=None, ctx=None, method="embedding"):
    """Balanced truncation's guarantee, measured: max_k ‖H(iω_k) - H_r(iω_k)‖₂ of the full system against the ReducedModel `rom`, both
    frequency responses from the device -> dict(max_error, omega_at_max, bound = 2 Σ_{i>r} hsv_i, ratio = bound / max_error).  method: as
    `freq_response` ("complex" serves n <= 4096 at half the flops)."""
    if not isinstance(rom, ReducedModel):
        raise TypeError(f"bt_error: rom must be a ReducedModel, not {type(rom).__name__}; nothing was run on the device")
    name = "bt_error"
    mats, w, _ = _freq_check(name, [(E, A, B, C)], omega, None, "raise", chunk, method)
    if (rom.Br.shape[1], rom.Cr.shape[0]) != (mats[0][2].shape[1], mats[0][3].shape[0]):
        raise ValueError(f"{name}: the reduced model has (m, q) = {(rom.Br.shape[1], rom.Cr.shape[0])}, the system "
                         f"{(mats[0][2].shape[1], mats[0][3].shape[0])}; nothing was run on the device")
    H = freq_response(E, A, B, C, w, chunk=chunk, ctx=ctx, method=method)
    Hr = rom.freq_response(w, chunk=chunk, ctx=ctx, method=method)
    err = np.linalg.svd(H - Hr, compute_uv=False)[:, 0]
    k = int(np.argmax(err))
    bound = 2.0 * float(np.sum(np.asarray(rom.hsv, dtype=float)[rom.order:][::-1]))
    return dict(max_error=float(err[k]), omega_at_max=float(w[k]), bound=bound, ratio=bound / float(err[k]) if err[k] > 0 else math.inf)


# ------------------------------------------------------------------------------------------------
# Time response: step, impulse, simulate                                    csrc/time_response.hip
# ------------------------------------------------------------------------------------------------
TIME_METHODS = ("tustin", "backward_euler")
TIME_SIMULATE_MAX_Q, TIME_SIMULATE_MAX_QM = 256, 2048     # TR_CONV_MAX_Q, TR_CONV_MAX_QM of csrc/time_response.hpp


def _time_check(name, E, A, B, C, dt, steps, D, method, block):
    """the argument errors of the time-response calls, before anything runs on the device -> ((E, A, B, C), dt, D)"""
    if method not in TIME_METHODS:
        raise ValueError(f"{name}: method must be 'tustin' (order 2, A-stable) or 'backward_euler' (order 1, L-stable; the choice for a singular "
                         f"E), got {method!r}; nothing was run on the device")
    if isinstance(dt, (bool, np.bool_)) or not isinstance(dt, (int, float, np.integer, np.floating)):
        raise TypeError(f"{name}: dt must be a number, not {type(dt).__name__}; nothing was run on the device")
    if not np.isfinite(dt) or dt <= 0:
        raise ValueError(f"{name}: dt must be finite and positive, got {dt!r}; nothing was run on the device")
    if isinstance(steps, (bool, np.bool_)) or not isinstance(steps, (int, np.integer)):
        raise TypeError(f"{name}: the number of steps must be an int, not {type(steps).__name__}; nothing was run on the device")
    if steps < 1:
        raise ValueError(f"{name}: at least one time step is needed, got {steps}; nothing was run on the device")
    if block is not None and (isinstance(block, (bool, np.bool_)) or not isinstance(block, (int, np.integer)) or block < 1 or block & (block - 1)):
        raise ValueError(f"{name}: block must be None (the default block length) or a power of two (1: plain sequential stepping), got {block!r}; "
                         "nothing was run on the device")
    ms = []
    for nm, M in zip("EABC", (E, A, B, C)):
        if not isinstance(M, (np.ndarray, LowRankUpdate, ScaledPencil)) and not sp.issparse(M):
            raise TypeError(f"{name}: {nm} must be a matrix, not {type(M).__name__}; nothing was run on the device")
        ms.append(_dense_f64(_dense_operator(M)))
    Ed, Am, Bm, Cm = ms
    n = Ed.shape[0] if Ed.ndim == 2 else 0
    if Ed.ndim != 2 or Ed.shape != (n, n) or Am.shape != (n, n) or Bm.ndim != 2 or Bm.shape[0] != n or Cm.ndim != 2 or Cm.shape[1] != n \
            or n < 1 or Bm.shape[1] < 1 or Cm.shape[0] < 1:
        raise ValueError(f"{name}: E and A must be n x n, B n x m and C q x n (n, m, q >= 1); got {Ed.shape}, {Am.shape}, {Bm.shape}, {Cm.shape}; "
                         "nothing was run on the device")
    if D is not None:
        D = np.asarray(D, dtype=float)
        if D.shape != (Cm.shape[0], Bm.shape[1]):
            raise ValueError(f"{name}: D must be q x m = {(Cm.shape[0], Bm.shape[1])}, got {D.shape}; nothing was run on the device")
    return (Ed, Am, Bm, Cm), float(dt), D


def _time_run(mats, method, dt, K, kind, U, X0, block, ctx):
    """one dre_time_response call -> (Y flat, info)"""
    ctx = ctx or dev.default_context()
    n, m, q = mats[0].shape[0], mats[2].shape[1], mats[3].shape[0]
    S = U.shape[0] if kind == 2 else 0
    ups = [ctx.upload(M) for M in mats]
    Y = np.zeros((S * (K + 1) * q) if kind == 2 else ((K + 1) * q * m))
    info = (C.c_int64 * 4)()
    pd = C.POINTER(C.c_double)
    Up = np.ascontiguousarray(U, dtype=float).ctypes.data_as(pd) if kind == 2 else None        # (S, K+1, m) C-ordered: u_k[c] of s at s (K+1) m + k m + c
    Xc = np.ascontiguousarray(X0, dtype=float) if X0 is not None else None                      # (S, n) C-ordered = n x S column-major
    ctx.chk(ctx.lib.dre_time_response(ctx.ptr, *(u.ptr for u in ups), TIME_METHODS.index(method), dt, int(K), kind, Up, S,
                                      Xc.ctypes.data_as(pd) if Xc is not None else None, int(block or 0), Y.ctypes.data_as(pd), info))
    return Y, dict(block=int(info[0]), blocks=int(info[1]), squarings=int(info[2]), launches=int(info[3]), method=method, order=n)


def step_response(E, A, B, C, dt, steps, D=None, method="tustin", block=None, ctx=None, return_info=False):
    """The step response of the dense descriptor system E ẋ = A x + B u, y = C x + D u on t_k = k dt, k = 0 .. steps, on the device
    (`dre_time_response`): a real array (steps + 1, q, m), entry [k, :, c] the output at t_k for a unit step on input channel c from x(0) = 0.
    method="tustin" (default; order 2, A-stable): x_{k+1} = M x_k + N (u_k + u_{k+1}) with P = E − (dt/2) A, M = 2 P⁻¹E − I, N = (dt/2) P⁻¹B;
    method="backward_euler" (order 1, L-stable): P = E − dt A, M = P⁻¹E, N = dt P⁻¹B, input u_{k+1}.  E may be singular; tustin then has the
    eigenvalue −1 on the algebraic part (it never decays), so backward_euler is the method for a singular E.  The pencil need not be stable:
    a growing response is a valid result.  The outputs come from the Markov sequence C Mʲ, built by doubling up to the block length and then
    `block` samples per GEMM, not from `steps` dependent thin products; block=None: the power of two at which one such GEMM fills the device
    (`tr_default_block` of csrc/time_response.hpp); block=1: plain sequential stepping.  D (q x m) is added on the host.  A call is bit for bit repeatable.  return_info=True appends dict(block,
    blocks, squarings, launches, method, order).  A singular P (dt on a pole of the scheme, a NaN in E or A) is DREError(-4).  Wrong types and
    shapes, a non-finite or non-positive dt, steps < 1, an unknown method and a block that is not a power of two are errors before anything
    runs on the device."""
    name = "step_response"
    mats, dt, D = _time_check(name, E, A, B, C, dt, steps, D, method, block)
    Y, info = _time_run(mats, method, dt, steps, 0, None, None, block, ctx)
    Y = Y.reshape(steps + 1, mats[2].shape[1], mats[3].shape[0]).transpose(0, 2, 1)      # samples hold q x m column-major
    Y = np.ascontiguousarray(Y) if D is None else Y + D
    return (Y, info) if return_info else Y


def impulse_response(E, A, B, C, dt, steps, method="tustin", block=None, ctx=None, return_info=False):
    """The impulse response on t_k = k dt, k = 0 .. steps: a real array (steps + 1, q, m), the free response y_k = C Mᵏ E⁻¹B from
    x(0+) = E⁻¹B under the one-step scheme `method` (see `step_response`, whose other arguments and errors this call shares).  E must be
    regular: a singular E is DREError(-4).  A feedthrough D is not added: a Dirac impulse has no sample."""
    name = "impulse_response"
    mats, dt, _ = _time_check(name, E, A, B, C, dt, steps, None, method, block)
    Y, info = _time_run(mats, method, dt, steps, 1, None, None, block, ctx)
    Y = np.ascontiguousarray(Y.reshape(steps + 1, mats[2].shape[1], mats[3].shape[0]).transpose(0, 2, 1))
    return (Y, info) if return_info else Y


def simulate(E, A, B, C, u, dt, x0=None, D=None, method="tustin", block=None, ctx=None, return_info=False):
    """The output of E ẋ = A x + B u, y = C x + D u for given input samples u_k = u(k dt) and initial state x0, on the device: u of shape
    (K+1, m) -> (K+1, q); u of shape (S, K+1, m) -> (S, K+1, q), S input signals ("scenarios") in one call; x0 of shape (n,) (shared) or
    (S, n), None: zero.  y_k = C Mᵏ x_0 + Σ_{j<k} h_j w_{k−1−j} + D u_k with h_j = C Mʲ N and w_k = u_k + u_{k+1} (tustin) or u_{k+1}
    (backward_euler): a causal convolution with the Markov parameters, K² q m S / 2 multiply-adds beside the GEMMs of `step_response`, whose
    other arguments and errors this call shares.  Limits: q <= 256 and q m <= 2048.  A non-finite u or x0 is an error before anything runs on
    the device."""
    name = "simulate"
    if not isinstance(u, (np.ndarray, list, tuple)):
        raise TypeError(f"{name}: u must be an array of input samples, not {type(u).__name__}; nothing was run on the device")
    try:
        ua = np.asarray(u, dtype=float)
    except (TypeError, ValueError):
        raise TypeError(f"{name}: u must be a real array of input samples; nothing was run on the device") from None
    if ua.ndim not in (2, 3):
        raise ValueError(f"{name}: u must have shape (K+1, m) or (S, K+1, m), got {ua.shape}; nothing was run on the device")
    single = ua.ndim == 2
    U = ua[None] if single else ua
    S, K = U.shape[0], U.shape[1] - 1
    mats, dt, D = _time_check(name, E, A, B, C, dt, K, D, method, block)
    n, m, q = mats[0].shape[0], mats[2].shape[1], mats[3].shape[0]
    if S < 1 or S > 65535 or U.shape[2] != m:
        raise ValueError(f"{name}: u must have shape (K+1, m) or (S, K+1, m) with m = {m} and 1 <= S <= 65535, got {ua.shape}; nothing was run on "
                         "the device")
    if not np.isfinite(U).all():
        raise ValueError(f"{name}: u has a non-finite entry; nothing was run on the device")
    X0 = None
    if x0 is not None:
        try:
            xa = np.asarray(x0, dtype=float)
        except (TypeError, ValueError):
            raise TypeError(f"{name}: x0 must be a real array; nothing was run on the device") from None
        if xa.shape not in ((n,), (S, n)):
            raise ValueError(f"{name}: x0 must have shape (n,) or (S, n) = {(n,)} or {(S, n)}, got {xa.shape}; nothing was run on the device")
        if not np.isfinite(xa).all():
            raise ValueError(f"{name}: x0 has a non-finite entry; nothing was run on the device")
        X0 = np.broadcast_to(xa, (S, n))
    if q > TIME_SIMULATE_MAX_Q or q * m > TIME_SIMULATE_MAX_QM:
        raise ValueError(f"{name}: the convolution kernel takes q <= {TIME_SIMULATE_MAX_Q} outputs and q m <= {TIME_SIMULATE_MAX_QM}, got q = {q}, "
                         f"m = {m}; nothing was run on the device")
    Y, info = _time_run(mats, method, dt, K, 2, U, X0, block, ctx)
    Y = Y.reshape(S, K + 1, q)
    if D is not None:
        Y = Y + U @ D.T
    Y = Y[0] if single else Y
    return (Y, info) if return_info else Y


# ------------------------------------------------------------------------------------------------
# LQG balanced truncation from one Hamiltonian sign iteration               csrc/dense_are.hip, csrc/balance.hip
# ------------------------------------------------------------------------------------------------
@dataclass
class LQGReducedModel:
    """ẋ_r = Ar x_r + Br u, y = Cr x_r (Er is the identity): the LQG balanced truncation of E ẋ = A x + B u, y = C x to order len(Ar); the plant
    need not be stable.  mu: the LQG characteristic values; T, W: the projections (Wᵀ E T = I); Kr, Lr, Ac: the reduced-order LQG controller
    ẋ_c = Ac x_c + Lr y, u = −Kr x_c with Kr = Brᵀ Σ_r, Lr = Σ_r Crᵀ, Ac = Ar − Br Kr − Lr Cr.  K: the full-order feedback BᵀXE that
    `lqg_error` needs (None for a model that was put together by hand)."""
    Er: np.ndarray
    Ar: np.ndarray
    Br: np.ndarray
    Cr: np.ndarray
    mu: np.ndarray
    T: np.ndarray
    W: np.ndarray
    Kr: np.ndarray
    Lr: np.ndarray
    Ac: np.ndarray
    K: np.ndarray | None = None

    @property
    def order(self):
        return self.Ar.shape[0]

    def controller(self):
        """(Ac, Lr, Kr) of ẋ_c = Ac x_c + Lr y, u = −Kr x_c"""
        return self.Ac, self.Lr, self.Kr

    def freq_response(self, omega, D=None, **kw):
        """H_r(iω) = Cr (iω I - Ar)⁻¹ Br (+ D) of the reduced model at every frequency of omega, on the device (as `ReducedModel.freq_response`;
        keywords as `freq_response`, method="embedding" | "complex" among them)."""
        return freq_response(self.Er, self.Ar, self.Br, self.Cr, omega, D=D, **kw)

    def step_response(self, dt, steps, D=None, **kw):
        """the step response of the reduced model on t_k = k dt, (steps + 1, q, m), on the device: `step_response` with E_r = I and its keywords"""
        return step_response(self.Er, self.Ar, self.Br, self.Cr, dt, steps, D=D, **kw)

    def impulse_response(self, dt, steps, **kw):
        """the impulse response of the reduced model, (steps + 1, q, m), on the device: `impulse_response` with E_r = I and its keywords"""
        return impulse_response(self.Er, self.Ar, self.Br, self.Cr, dt, steps, **kw)

    def simulate(self, u, dt, x0=None, D=None, **kw):
        """the reduced model's output for the input samples u (x0 in reduced coordinates), on the device: `simulate` with E_r = I and its keywords"""
        return simulate(self.Er, self.Ar, self.Br, self.Cr, u, dt, x0=x0, D=D, **kw)


def _lqg_check(name, E, A, B, C, alg, order, tol, Rinv=None, S=None):
    if not isinstance(alg, MatrixSign):
        raise TypeError(f"{name} takes alg = MatrixSign(), not {type(alg).__name__} (both Riccati solutions come from the dense Hamiltonian sign "
                        "iteration); nothing was run on the device")
    Eh, Ah, Bh, Ch = (_dense_f64(M) for M in _balance_check(name, E, A, B, C, alg, order, tol))
    n, m, q = Eh.shape[0], Bh.shape[1], Ch.shape[0]
    if n < 1 or m < 1 or q < 1:
        raise ValueError(f"{name}: n, m and q must be at least 1; got E {Eh.shape}, B {Bh.shape}, C {Ch.shape}; nothing was run on the device")
    inner = []
    for nm, M, k in (("Rinv", Rinv, m), ("S", S, q)):
        if M is not None:
            M = np.asarray(M, dtype=float)
            if M.shape != (k, k):
                raise ValueError(f"{name}: {nm} must be {k} x {k}, got {M.shape}; nothing was run on the device")
            M = _dense_f64(M)
        inner.append(M)
    return Eh, Ah, Bh, Ch, inner[0], inner[1]


def _gare_pair_device(ctx, alg, Ed, Ad, Bd, Ctd, Rd=None, Sd=None):
    """`dre_dense_gare_solve_pair` on uploaded operands -> (X, Y) as device matrices and the info dict"""
    maxiters, tol, max_refine = _sign_params(alg)
    xp, yp = C.c_void_p(), C.c_void_p()
    ii, dd = (C.c_int64 * 4)(), (C.c_double * 4)()
    ptr = lambda u: u.ptr if u is not None else None                          # noqa: E731
    ctx.chk(ctx.lib.dre_dense_gare_solve_pair(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, ptr(Rd), Ctd.ptr, ptr(Sd), maxiters, tol, max_refine, C.byref(xp),
                                              C.byref(yp), ii, dd))
    info = dict(iters=int(ii[0]), factorizations=1, regulator=dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1])),
                filter=dict(iters=int(ii[2]), refinements=int(ii[3]), res0=float(dd[2]), res=float(dd[3])))
    return dev.DenseMatrix(ctx, xp), dev.DenseMatrix(ctx, yp), info


def solve_gare_pair(E, A, B, C, alg=MatrixSign(), Rinv=None, S=None, ctx=None, return_info=False):
    """Both Riccati equations of LQG design from ONE sign iteration of the Hamiltonian pencil (`dre_dense_gare_solve_pair`) -> (X, Y):
        AᵀXE + EᵀXA − EᵀXGXE + Q = 0   (regulator)        A Y Eᵀ + E Y Aᵀ − E Y Q Y Eᵀ + G = 0   (filter)        G = B R⁻¹ Bᵀ, Q = Cᵀ S C
    (Rinv m x m and S q x q: None is the identity).  X is bit for bit what solve(GAREProblem(E, A, G, Q), MatrixSign()) returns; Y comes from
    the transposed blocks of the same sign matrix and is refined on the dual closed loop A − E Y Q.  Open-loop unstable plants are fine as
    long as (A, B, E) is stabilizable and (A, C, E) detectable.  return_info=True adds dict(iters, factorizations=1, regulator=dict(iters,
    refinements, res0, res), filter=the same).  Wrong types and shapes are errors before anything runs on the device."""
    name = "solve_gare_pair"
    Eh, Ah, Bh, Ch, Rh, Sh = _lqg_check(name, E, A, B, C, alg, None, 0.0, Rinv, S)
    ctx = ctx or dev.default_context()
    ups = [ctx.upload(M) if M is not None else None for M in (Eh, Ah, Bh, np.asfortranarray(Ch.T), Rh, Sh)]
    X, Y, info = _gare_pair_device(ctx, alg, *ups)
    X, Y = X.numpy(), Y.numpy()
    return ((X, Y), info) if return_info else (X, Y)


def _lqg_balance(name, E, A, B, Cout, alg, order, tol, ctx):
    Eh, Ah, Bh, Ch, _, _ = _lqg_check(name, E, A, B, Cout, alg, order, tol)
    ctx = ctx or dev.default_context()
    Ed, Ad, Bd, Cd, Ctd = (ctx.upload(M) for M in (Eh, Ah, Bh, Ch, np.asfortranarray(Ch.T)))
    X, Y, pair = _gare_pair_device(ctx, alg, Ed, Ad, Bd, Ctd)
    out = [C.c_void_p() for _ in range(9)]
    ii, dd = (C.c_int64 * 6)(), (C.c_double * 3)()
    ctx.chk(ctx.lib.dre_lqg_balance(ctx.ptr, Ed.ptr, Ad.ptr, Bd.ptr, Cd.ptr, X.ptr, Y.ptr, int(order or 0), float(tol), *(C.byref(p) for p in out), ii, dd))
    mu, T, W, Ar, Br, Cr, Kr, Lr, Ac = (dev.DenseMatrix(ctx, p).numpy() for p in out)
    info = dict(regulator=pair["regulator"], filter=pair["filter"], iters=pair["iters"], factorizations=1, order=int(ii[0]), rank=int(ii[1]),
                r_c=int(ii[2]), r_o=int(ii[3]), dropped=int(ii[4]), svd_sweeps=int(ii[5]), eye_err=float(dd[0]), bound=float(dd[1]), neg_max=float(dd[2]))
    K = Bh.T @ X.numpy() @ Eh
    return LQGReducedModel(np.eye(Ar.shape[0]), Ar, Br, Cr, mu.ravel(), T, W, Kr, Lr, Ac, K), info


def lqg_balanced_truncation(E, A, B, C, alg=MatrixSign(), order=None, tol=1e-8, ctx=None, return_info=False):
    """LQG balanced truncation of E ẋ = A x + B u, y = C x on the device -> LQGReducedModel.  The pencil (A, E) need not be c-stable (only
    stabilizable and detectable): instead of the Gramians the stabilizing solutions X and Y of the regulator and the filter Riccati equations
    are balanced, and both come from ONE Hamiltonian sign iteration (`dre_dense_gare_solve_pair`).  `dre_lqg_balance` factors them, runs the
    steps of `balanced_truncation` and adds the reduced-order LQG controller.
    order: the reduced order (above the numerical rank: DREError(-1)); None: the smallest r with 2 Σ_{i>r} ν_i <= tol, ν_i = μ_i / √(1 + μ_i²)
    (absolute: it bounds the error of the normalised right coprime factors, whose norm is 1).
    return_info=True adds dict(iters, factorizations=1, regulator, filter (each dict(iters, refinements, res0, res)), order, rank, r_c, r_o,
    dropped, svd_sweeps, eye_err = ||WᵀET - I||_F, bound = 2 Σ_{i>r} ν_i, neg_max).  Wrong types and shapes are errors before anything runs
    on the device."""
    red, info = _lqg_balance("lqg_balanced_truncation", E, A, B, C, alg, order, tol, ctx)
    return (red, info) if return_info else red


def lqg_characteristic_values(E, A, B, C, alg=MatrixSign(), ctx=None):
    """The LQG characteristic values of E ẋ = A x + B u, y = C x, descending: the square roots of the eigenvalues of Y EᵀX E (the `mu` of
    `lqg_balanced_truncation`)."""
    return _lqg_balance("lqg_characteristic_values", E, A, B, C, alg, None, 0.0, ctx)[0].mu


def lqg_error(E, A, B, C, rom, omega, chunk=None, ctx=None, method="embedding"):
    """LQG balanced truncation's guarantee, measured -> (err, bound): err = max_k ‖[N; M](iω_k) − [N_r; M_r](iω_k)‖₂ of the normalised right
    coprime factors of the plant and of the LQGReducedModel `rom`, from two `freq_response` calls on (E, A − BK, B, [C; −K]) with
    D = [0; I], K = BᵀXE, and on (I, Ar − Br Kr, Br, [Cr; −Kr]); bound = 2 Σ_{i>r} μ_i / √(1 + μ_i²).  K is taken from `rom`; a model
    without it costs one regulator solve.  method: as `freq_response` ("complex" serves n <= 4096 at half the flops)."""
    name = "lqg_error"
    if not isinstance(rom, LQGReducedModel):
        raise TypeError(f"{name}: rom must be an LQGReducedModel, not {type(rom).__name__}; nothing was run on the device")
    mats, w, _ = _freq_check(name, [(E, A, B, C)], omega, None, "raise", chunk, method)
    Eh, Ah, Bh, Ch = mats[0]
    m, q = Bh.shape[1], Ch.shape[0]
    if (rom.Br.shape[1], rom.Cr.shape[0]) != (m, q):
        raise ValueError(f"{name}: the reduced model has (m, q) = {(rom.Br.shape[1], rom.Cr.shape[0])}, the system {(m, q)}; nothing was run on the device")
    K = rom.K
    if K is None:
        K = Bh.T @ solve_gare_pair(Eh, Ah, Bh, Ch, ctx=ctx)[0] @ Eh
    Dn = np.vstack([np.zeros((q, m)), np.eye(m)])
    H = freq_response(Eh, Ah - Bh @ K, Bh, np.vstack([Ch, -K]), w, D=Dn, chunk=chunk, ctx=ctx, method=method)
    Hr = freq_response(rom.Er, rom.Ar - rom.Br @ rom.Kr, rom.Br, np.vstack([rom.Cr, -rom.Kr]), w, D=Dn, chunk=chunk, ctx=ctx, method=method)
    err = float(np.linalg.svd(H - Hr, compute_uv=False)[:, 0].max())
    mu = np.asarray(rom.mu, dtype=float)[rom.order:]
    return err, 2.0 * float(np.sum((mu / np.sqrt(1.0 + mu * mu))[::-1]))


def _solve_gdre_factored_sign(prob, alg, order, inner, dt, save_state, observer, ctx, return_stats):
    """solve(::GDREProblem{<:LDLᵀ}, ::Ros1/Ros2(FactoredSign()); dt, save_state, observer): the host-driven Rosenbrock loop with one kept sign
    factorisation per time step and one factored replay per stage.  The observe_gdre_* hooks fire as on the other paths; there are no ADI
    iterations to report."""
    Ed = ctx.upload(_dense_f64(prob.E))
    n = Ed.shape[0]
    maxiters, tol, rtol, max_width, max_refine = _factored_sign_params(inner, n)
    solves = []
    live = []                       # the current step's factorisation: (maxiters + 7) n² doubles, released before the next one is made

    def step_solver(F):
        while live:
            live.pop().close()
        sign = SignFactorization(Ed, F, maxiters, tol if tol > 0 else None, ctx)
        live.append(sign)

        def lyap(rhs, guess):
            X, info = solve_gale_factored_sign(GALEProblem(prob.E, F, rhs), inner, ctx, True, _sign=sign)
            solves.append(info)
            return X
        return lyap

    try:
        sol = _rosenbrock_lowrank_loop(prob, alg, order, dt, save_state, observer, step_solver)
    finally:
        while live:
            live.pop().close()
    if return_stats:
        return sol, dict(lyapunov_solves=len(solves), solves=solves, ranks=[X.rank() for X in sol.X])
    return sol


# ------------------------------------------------------------------------------------------------
# Low-rank FGMRES with (optional) ADI preconditioner                                   
# src/lyapunov/gmres.jl:7-134, src/lyapunov/types.jl:44-52, dot: src/LDLt.jl:91-108
# ------------------------------------------------------------------------------------------------
@dataclass
class GMRES:
    """Flexible GMRES options (lyapunov/types.jl:44-52)."""
    maxiters: int = 3            # per restart
    maxrestarts: int = 0
    reltol: Optional[float] = None
    abstol: Optional[float] = None
    ignore_initial_guess: bool = False
    compression: bool = True
    preconditioner: Any = None
    warn_convergence: bool = True


def dot(X1: LDLt, X2: LDLt, ctx=None, pencil=None) -> float:
    """dot(::LDLᵀ, ::LDLᵀ) = <X1, X2>_F  (LDLt.jl:91-108).  With a pencil (or operands that already live on one) the Gram products run on
    the device (dre_ldlt_dot); plain host objects without a pencil fall back to small host GEMMs on the factors."""
    if pencil is None:
        for X in (X1, X2):
            if X._handle is not None and X._handle.pencil is not None:
                pencil = X._handle.pencil
    if pencil is not None:
        ctx = ctx or pencil.ctx
        h1, h2 = X1._to_device(ctx, pencil), X2._to_device(ctx, pencil)
        out = C.c_double()
        ctx.chk(ctx.lib.dre_ldlt_dot(ctx.ptr, h1.ptr, h2.ptr, C.byref(out)))
        return out.value
    a, A, Bm = X1
    b, Cm, Dm = X2
    M = A.T @ Cm
    return float(a * b * np.sum((Bm @ M @ Dm) * M))


def _opT_mul(A, Z):
    """A' Z for a sparse matrix or a LowRankUpdate  A0 + inv(alpha) U V  (LowRankUpdate.jl:51-54,82-85)."""
    if isinstance(A, LowRankUpdate):
        return _spT_mul(A.A, Z) + np.asarray(A.V).T @ (np.asarray(A.U).T @ Z) / A.alpha
    return _spT_mul(A, Z)


def lyapunov_apply(E, A, X: LDLt, ctx=None) -> LDLt:
    """LyapunovOperator(E, A) * X = A'XE + E'XA = a [E'Z, A'Z] [0 Y; Y 0] [E'Z, A'Z]'  (gmres.jl:108-120).  On the device when a context is
    given (dre_gale_apply: two SpMMs + the rank-m part of a LowRankUpdate), host NumPy otherwise."""
    if ctx is not None:
        A0, lr = _split_operator(E, A)
        pencil = _pencil_for(E, A0, ctx)
        Xd = X._to_device(ctx, pencil)
        U = Vt = None
        alpha = 1.0
        if lr is not None:
            alpha, Uh, Vh = lr
            U, Vt = ctx.upload(Uh), ctx.upload(np.asarray(Vh).T)
        out = C.c_void_p()
        ctx.chk(ctx.lib.dre_gale_apply(ctx.ptr, pencil.ptr, 1.0, 0.0, float(alpha), U.ptr if U else None, Vt.ptr if Vt else None, Xd.ptr, C.byref(out)))
        return LDLt([], [], [], _handle=dev.DeviceLDLt(ctx, out, pencil))
    a, Z, Y = X
    O = np.zeros_like(Y)
    return a * lowrank(np.hstack([_spT_mul(E, Z), _opT_mul(A, Z)]), np.block([[O, Y], [Y, O]]))


def _specialize(alg, prob, ctx):
    """gmres.jl:122-134: the Heuristic shifts of a preconditioner are computed once per problem, not once per inner solve."""
    if isinstance(alg, ADI) and isinstance(alg.shifts, Shifts.Cyclic) and isinstance(alg.shifts.inner, Shifts.Heuristic):
        A0, lr = _split_operator(prob.E, prob.A)
        return dataclasses.replace(alg, shifts=Shifts.Cyclic(heuristic_shifts(alg.shifts.inner, _pencil_for(prob.E, A0, ctx), lr)))
    if isinstance(alg, GMRES):
        return dataclasses.replace(alg, preconditioner=_specialize(alg.preconditioner, prob, ctx))
    return alg


def solve_gmres(prob: GALEProblem, alg: GMRES, initial_guess: LDLt | None = None, abstol=None, observer=None, ctx=None, return_info=False):
    """solve(::GALEProblem, ::GMRES; initial_guess, abstol, observer)  (lyapunov/gmres.jl:7-106): flexible GMRES (Saad 1993, Alg. 2.2) on
    low-rank iterates.  The Arnoldi bookkeeping is host logic as in the reference; residuals, compressions, norms and the ADI
    preconditioner solves run on the device."""
    ctx = ctx or dev.default_context()
    _call(observer, "observe_gale_start", prob, alg)
    E, A, Cl = prob.E, prob.A, prob.C
    X = Cl.zero() if (alg.ignore_initial_guess or initial_guess is None) else initial_guess
    reltol = alg.reltol if alg.reltol is not None else Cl.n * np.finfo(float).eps
    if abstol is None:
        abstol = alg.abstol if alg.abstol is not None else reltol * norm(Cl)
    pre = _specialize(alg.preconditioner, prob, ctx)
    mmax = alg.maxiters
    H, bvec = np.zeros((mmax + 1, mmax)), np.zeros(mmax + 1)
    residual_norm, m, restarts = math.inf, 0, 0
    for restarts in range(alg.maxrestarts + 1):
        m = 0
        R0 = residual(prob, X, ctx)
        beta = residual_norm = norm(R0)
        _call(observer, "observe_gale_step", 0, X, R0, beta)
        if beta <= abstol:
            break
        V, Zs = [R0 / beta], []
        H[:] = 0.0; bvec[:] = 0.0; bvec[0] = beta
        y = np.zeros(0)
        for j in range(mmax):
            if pre is None:
                Zs.append(V[j])
            else:
                sub = GALEProblem(E, A, V[j])
                Zs.append(solve_gale(sub, pre, observer=observer, ctx=ctx) if isinstance(pre, ADI) else solve_gmres(sub, pre, observer=observer, ctx=ctx))
            W = lyapunov_apply(E, A, Zs[j], ctx)       # device: dre_gale_apply
            if alg.compression:
                compress_(W)
            for i in range(j + 1):
                H[i, j] = dot(V[i], W, ctx)            # device: dre_ldlt_dot
                W = W - H[i, j] * V[i]
            H[j + 1, j] = norm(W)
            V.append(W / H[j + 1, j])
            m = j + 1
            Hm, bm = H[:m + 1, :m], bvec[:m + 1]
            y = np.linalg.lstsq(Hm, bm, rcond=None)[0]
            residual_norm = float(np.linalg.norm(bm - Hm @ y))
            if residual_norm <= abstol:
                break
            _call(observer, "observe_gale_step", m, None, None, residual_norm)
            if alg.compression:
                compress_(V[j + 1])
        for j in range(m):
            X = X + (-y[j]) * Zs[j]
        if alg.compression:
            compress_(X)
        _call(observer, "observe_gale_step", m, X, None, residual_norm)
        if residual_norm <= abstol:
            break
    iters = restarts * alg.maxiters + m
    if residual_norm > abstol:
        _call(observer, "observe_gale_failed")
        if alg.warn_convergence:
            warnings.warn(f"GMRES did not converge: residual={residual_norm} abstol={abstol} maxrestarts={alg.maxrestarts} maxiters={alg.maxiters}")
    _call(observer, "observe_gale_done", iters, X, None, residual_norm)
    if return_info:
        return X, dict(iters=iters, res_norm=residual_norm, abstol=abstol, converged=residual_norm <= abstol)
    return X


# ------------------------------------------------------------------------------------------------
# Algebraic Riccati equation: Kleinman-Newton with the device ADI as inner solver     
# src/riccati/types.jl:41-107, src/riccati/newton.jl:3-172, src/riccati/residual.jl:5-52
# ------------------------------------------------------------------------------------------------
@dataclass
class GAREProblem:
    """Q + A'XE + E'XA − E'XGXE = 0 with G = lowrank(B, I), Q = lowrank(C', I) (riccati/types.jl:41-52)."""
    E: Any
    A: Any
    G: LDLt
    Q: LDLt


def quadratic_forcing(_, residual_norm):          # newton.jl:164-172
    return min(0.1, 0.9 * residual_norm)


def superlinear_forcing(i, _):                    # newton.jl:150-157
    return 1.0 / (i ** 3 + 1)


@dataclass
class Newton:
    """Kleinman-Newton options (riccati/types.jl:96-107)."""
    inner_alg: Optional[ADI] = None
    maxiters: int = 5
    reltol: Optional[float] = None
    abstol: Optional[float] = None
    inexact: bool = True
    inexact_hybrid: bool = True
    inexact_forcing: Any = quadratic_forcing
    linesearch: bool = True


def _spT_mul(M, L):
    return np.asarray(M.T @ L) if sp.issparse(M) else np.asarray(M).T @ L


def gare_residual(prob: GAREProblem, X: LDLt, ctx=None, drop_below=None) -> LDLt:
    """residual(::GAREProblem, ::LDLᵀ)  (riccati/residual.jl:5-52): the factors R = [C', A'L, E'L] and the small T are assembled on
    the DEVICE from the factors of X (dre_gare_residual) and compressed there; nothing of size n x rank crosses the bus."""
    if X.iszero():
        g, Ct, S = prob.Q
        return g * lowrank(Ct.copy(), np.array(S, dtype=float))
    gamma, Ct, S = prob.Q
    beta, B, Rinv = prob.G
    ctx = ctx or dev.default_context()
    pencil = _pencil_for(prob.E, prob.A, ctx)
    hx = X._to_device(ctx, pencil)                   # the factors of X stay where the ADI left them (no download of L)
    Ctd, Sd = ctx.upload(np.asarray(Ct, dtype=float)), ctx.upload(np.asarray(S, dtype=float))
    Bd, Rd = ctx.upload(np.asarray(B, dtype=float)), ctx.upload(np.asarray(Rinv, dtype=float))
    out = C.c_void_p()
    ctx.chk(ctx.lib.dre_gare_residual(ctx.ptr, pencil.ptr, hx.ptr, Ctd.ptr, Sd.ptr, float(gamma), Bd.ptr, Rd.ptr, float(beta), C.byref(out)))
    h = dev.DeviceLDLt(ctx, out, pencil)             # [C', A'L, E'L] T [...]' assembled on the device (dre_gare_residual)
    h.compress(drop_below)                           # drop_below: absolute truncation (the Newton loop passes a fraction of its tolerance)
    return LDLt([], [], [], _handle=h)


def gare_feedback(prob: GAREProblem, X: LDLt, ctx=None) -> np.ndarray:
    """K = B'XE (newton.jl:104-112) from the device factors of X (dre_ldlt_feedback); only the m x n result comes back."""
    beta, B, Rinv = prob.G
    n = prob.A.shape[0]
    if X.rank() == 0:
        return np.zeros((B.shape[1], n))
    ctx = ctx or dev.default_context()
    pencil = _pencil_for(prob.E, prob.A, ctx)
    hx = X._to_device(ctx, pencil)
    Bd = ctx.upload(np.asarray(B, dtype=float))
    out = C.c_void_p()
    ctx.chk(ctx.lib.dre_ldlt_feedback(ctx.ptr, pencil.ptr, hx.ptr, Bd.ptr, C.byref(out)))
    return np.ascontiguousarray(dev.DenseMatrix(ctx, out).numpy().T)


def solve_gare(prob: GAREProblem, alg: Newton, observer=None, ctx=None, return_info=False):
    """solve(::GAREProblem, ::Newton; observer)  (riccati/newton.jl:3-147).  The Newton loop, the forcing terms and the Armijo line search
    are host logic exactly as in the reference; every Newton step is one device-resident LDLᵀ-ADI solve of
    (A − BK)'XE + E'X(A − BK) = −[C', E'XB][C', E'XB]' with the previous iterate as initial guess."""
    inner = alg.inner_alg if alg.inner_alg is not None else ADI()
    a_g, B, Dg = prob.G
    a_q, Ct, Dq = prob.Q
    if not (a_g == 1 and a_q == 1 and np.array_equal(Dg, np.eye(Dg.shape[0])) and np.array_equal(Dq, np.eye(Dq.shape[0]))):
        raise NotImplementedError("G and Q must be unscaled with identity inner matrices (newton.jl:8-9,15-17)")
    _call(observer, "observe_gare_start", prob, alg)
    n = prob.A.shape[0]
    res_norm = norm(prob.Q)
    reltol = alg.reltol if alg.reltol is not None else n * np.finfo(float).eps
    abstol = alg.abstol if alg.abstol is not None else reltol * res_norm
    inner_reltol = inner.reltol if inner.reltol is not None else reltol / 10
    X = lowrank(np.zeros((n, 0)), np.zeros((0, 0)))
    X_prev = None
    history, adi_iters, i = [], 0, 0

    def aux(Xc):
        return gare_feedback(prob, Xc, ctx)              # K = B'XE, formed on the device

    while True:
        K = aux(X)
        res = gare_residual(prob, X, ctx, drop_below=1e-3 * abstol)
        res_norm_prev, res_norm = res_norm, norm(res)
        if i > 0 and alg.linesearch and res_norm > (1 - 0.1) * res_norm_prev:      # Armijo, newton.jl:50-92
            Xt, lam = X, 0.5
            while True:
                X = (1 - lam) * X_prev + lam * Xt
                res = gare_residual(prob, X, ctx, drop_below=1e-3 * abstol)
                res_norm = norm(res)
                if res_norm < (1 - lam * 0.1) * res_norm_prev:
                    K = aux(X)
                    break
                lam *= 0.5
                if lam < np.finfo(float).eps:
                    warnings.warn("Line search failed; using un-modified iterate")
                    X, lam = Xt, 1.0
                    K = aux(X)
                    break
            _call(observer, "observe_gare_metadata", "line search", lam)
        _call(observer, "observe_gare_step", i, X, res, res_norm)
        history.append(res_norm)
        if res_norm <= abstol:
            break
        if i >= alg.maxiters:
            _call(observer, "observe_gare_failed")
            warnings.warn(f"Newton method did not converge: residual={res_norm} abstol={abstol} maxiters={alg.maxiters}")
            break
        i += 1
        F = lr_update(prob.A, -1.0, B, K)                                        # newton.jl:104
        G = np.hstack([Ct, K.T])                                                 # newton.jl:107-112  (E'XB = K')
        lyap = GALEProblem(prob.E, F, lowrank(G, np.eye(G.shape[1])))
        if alg.inexact:                                                          # newton.jl:116-133
            inner_abstol = alg.inexact_forcing(i, res_norm) * res_norm
            if alg.inexact_hybrid:
                classical = inner_reltol * norm(lyap.C)
                switch_back = classical > inner_abstol
                _call(observer, "observe_gare_metadata", "inexact", not switch_back)
                if switch_back:
                    inner_abstol = classical
            else:
                _call(observer, "observe_gare_metadata", "inexact", True)
        else:
            inner_abstol = inner_reltol * norm(lyap.C)
        X_prev = X
        if isinstance(inner, GMRES):
            X, info = solve_gmres(lyap, inner, initial_guess=X_prev, abstol=float(inner_abstol), observer=observer, ctx=ctx, return_info=True)
        else:
            X, info = solve_gale(lyap, dataclasses.replace(inner, abstol=float(inner_abstol)), initial_guess=X_prev, observer=observer,
                                 ctx=ctx, return_info=True)
        adi_iters += info["iters"]
    _call(observer, "observe_gare_done", i, X, res, res_norm)
    if return_info:
        return X, dict(newton_steps=i, residual_norms=history, abstol=abstol, adi_iters=adi_iters, converged=res_norm <= abstol)
    return X


def _gare_dense_operands(prob: GAREProblem, ctx):
    """E, A densified (as _dense_f64 does for the other dense solvers); G = beta B Rinv B' and Q = gamma C' S C stay factored: B, Ct and the
    inner matrices with the scalars folded in (None for an identity inner matrix with scalar 1)."""
    beta, B, Rinv = prob.G
    gamma, Ct, S = prob.Q
    B, Ct = _dense_f64(B), _dense_f64(Ct)
    Rinv, S = np.asarray(Rinv, dtype=float), np.asarray(S, dtype=float)
    Rs = None if beta == 1 and np.array_equal(Rinv, np.eye(B.shape[1])) else _dense_f64(beta * Rinv)
    Ss = None if gamma == 1 and np.array_equal(S, np.eye(Ct.shape[1])) else _dense_f64(gamma * S)
    ups = [ctx.upload(M) for M in (_dense_f64(prob.E), _dense_f64(prob.A), B, Ct)]
    ups += [ctx.upload(M) if M is not None else None for M in (Rs, Ss)]
    E, A, Bd, Ctd, Rd, Sd = ups
    ptr = lambda u: u.ptr if u is not None else None                          # noqa: E731
    return ups, (ptr(E), ptr(A), ptr(Bd), ptr(Rd), ptr(Ctd), ptr(Sd))


def solve_gare_dense(prob: GAREProblem, alg: MatrixSign, ctx=None, return_info=False):
    """solve(::GAREProblem, ::MatrixSign): the dense stabilizing solution X of Q + A'XE + E'XA − E'XGXE = 0 with G = β B R⁻¹ Bᵀ and
    Q = γ Cᵀ S C (any scalars and inner matrices), on the device: the sign function of the Hamiltonian pencil, extraction by Householder QR
    and up to alg.max_refine Newton-Kleinman steps (dre_dense_gare_solve).  Open-loop unstable plants are fine as long as (A, B, E) is
    stabilizable and (A, C, E) detectable; Hamiltonian eigenvalues on or near the imaginary axis raise DREError(-7).
    return_info: (X, dict(iters, refinements, res0, res, K)) with the scaled residuals ||R||_F / (||Q||_F + 2 ||A'XE||_F + ||E'XGXE||_F)
    after extraction and at the end, and the feedback K = R⁻¹BᵀXE (β folded in: K = β R⁻¹ Bᵀ X E)."""
    ctx = ctx or dev.default_context()
    keep, ptrs = _gare_dense_operands(prob, ctx)
    xp = C.c_void_p()
    ii, dd = (C.c_int64 * 2)(), (C.c_double * 2)()
    maxiters, tol, max_refine = _sign_params(alg)
    ctx.chk(ctx.lib.dre_dense_gare_solve(ctx.ptr, *ptrs, maxiters, tol, max_refine, C.byref(xp), ii, dd))
    X = dev.DenseMatrix(ctx, xp).numpy()
    del keep
    if return_info:
        beta, B, Rinv = prob.G
        E = prob.E.toarray() if sp.issparse(prob.E) else np.asarray(prob.E, dtype=float)
        K = (beta * np.asarray(Rinv, dtype=float)) @ (np.asarray(B, dtype=float).T @ X @ E)
        return X, dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1]), K=K)
    return X


def gare_residual_dense(prob: GAREProblem, X, ctx=None):
    """residual(::GAREProblem, X::Matrix)  (riccati/residual.jl:54-66) on the device: Q + A'XE + E'XA − E'XGXE (symmetrised) as an ndarray."""
    ctx = ctx or dev.default_context()
    keep, ptrs = _gare_dense_operands(prob, ctx)
    Xd = ctx.upload(_dense_f64(X))
    rp, nrm = C.c_void_p(), C.c_double()
    ctx.chk(ctx.lib.dre_dense_gare_residual(ctx.ptr, *ptrs, Xd.ptr, C.byref(rp), C.byref(nrm)))
    del keep
    return dev.DenseMatrix(ctx, rp).numpy()


# ------------------------------------------------------------------------------------------------
# Discrete time: the generalized Stein equation and the DARE by doubling          (csrc/dense_doubling.hip)
# ------------------------------------------------------------------------------------------------
@dataclass
class GDALEProblem:
    """AᵀXA − EᵀXE = −C (the generalized Stein equation, the discrete-time twin of GALEProblem); C an ndarray or an LDLᵀ object, as
    solve_gale_dense accepts it."""
    E: Any
    A: Any
    C: Any


@dataclass
class GDAREProblem:
    """Q + AᵀX(I + GX)⁻¹A − EᵀXE = 0, written out AᵀXA − EᵀXE − AᵀXB(R + BᵀXB)⁻¹BᵀXA + Q = 0, with G = lowrank(B, R⁻¹) and Q = lowrank(Cᵀ, S):
    the fields and the (β, B, Rinv) / (γ, Ct, S) conventions of GAREProblem."""
    E: Any
    A: Any
    G: LDLt
    Q: LDLt


@dataclass
class Doubling:
    """Dense discrete-time algorithm tag: the squared Smith iteration for a GDALEProblem and the structure-preserving doubling algorithm for
    a GDAREProblem, on the device.  The iteration runs at order n (any n up to 46340 whose 7 n² resp. 18 n² doubles fit in device memory).
    tol None: 10 n eps on the relative step ‖ΔH‖_F / ‖H‖_F (converged once that holds and ‖A_k‖_F < 1); max_refine: Newton (Hewer) steps of
    the DARE while the scaled residual exceeds 100 n eps and decreases (the Stein solver takes none).  A pencil with eigenvalues on or
    outside the unit circle (Stein), a symplectic pencil with eigenvalues on the unit circle or a plant that is not d-stabilizable (DARE)
    raise DREError(-7)."""
    maxiters: int = 50
    tol: Optional[float] = None
    max_refine: int = 2


def _doubling_check(name, alg):
    if not isinstance(alg, Doubling):
        raise TypeError(f"{name} takes alg = Doubling(), not {type(alg).__name__}; nothing was run on the device")
    if not (isinstance(alg.maxiters, (int, np.integer)) and 1 <= alg.maxiters <= 1000):
        raise ValueError(f"{name}: Doubling.maxiters must be an integer in 1 .. 1000, got {alg.maxiters!r}; nothing was run on the device")
    if not (isinstance(alg.max_refine, (int, np.integer)) and alg.max_refine >= 0):
        raise ValueError(f"{name}: Doubling.max_refine must be an integer >= 0, got {alg.max_refine!r}; nothing was run on the device")
    if alg.tol is not None and not (np.isfinite(alg.tol) and alg.tol > 0):
        raise ValueError(f"{name}: Doubling.tol must be None or a positive number, got {alg.tol!r}; nothing was run on the device")


def _square_pencil(name, E, A):
    E, A = _dense_f64(E), _dense_f64(A)
    n = E.shape[0] if E.ndim == 2 else 0
    if E.ndim != 2 or n < 1 or E.shape != (n, n) or A.shape != (n, n):
        raise ValueError(f"{name}: E and A must be square of the same order n >= 1, got {E.shape} and {A.shape}; nothing was run on the device")
    return E, A, n


def _gdale_operands(name, prob, X=None):
    if not isinstance(prob, GDALEProblem):
        raise TypeError(f"{name} takes a GDALEProblem, not {type(prob).__name__}; nothing was run on the device")
    E, A, n = _square_pencil(name, prob.E, prob.A)
    Cm = _dense_f64(prob.C.dense() if isinstance(prob.C, LDLt) else prob.C)
    if Cm.shape != (n, n):
        raise ValueError(f"{name}: C must be {n} x {n}, got {Cm.shape}; nothing was run on the device")
    if X is None:
        return E, A, Cm
    X = _dense_f64(X)
    if X.shape != (n, n):
        raise ValueError(f"{name}: X must be {n} x {n}, got {X.shape}; nothing was run on the device")
    return E, A, Cm, X


def _gdare_check(name, E, A, B, Ct, Rinv, S):
    """shapes of a DARE's operands (Ct is n x q) -> the dense f64 operands, Rinv and S None for the identity"""
    E, A, n = _square_pencil(name, E, A)
    B, Ct = _dense_f64(B), _dense_f64(Ct)
    if B.ndim != 2 or Ct.ndim != 2 or B.shape[0] != n or Ct.shape[0] != n or B.shape[1] < 1 or Ct.shape[1] < 1:
        raise ValueError(f"{name}: B must be {n} x m and C q x {n} with m, q >= 1, got B {B.shape} and C {Ct.T.shape}; nothing was run on the device")
    inner = []
    for nm, M, k in (("Rinv", Rinv, B.shape[1]), ("S", S, Ct.shape[1])):
        if M is not None:
            M = _dense_f64(M)
            if M.shape != (k, k):
                raise ValueError(f"{name}: {nm} must be {k} x {k}, got {M.shape}; nothing was run on the device")
        inner.append(M)
    return E, A, B, Ct, inner[0], inner[1]


def _gdare_operands(name, prob):
    """the checked host operands of a GDAREProblem with the scalars folded into the inner matrices (None: identity), as _gare_dense_operands"""
    if not isinstance(prob, GDAREProblem):
        raise TypeError(f"{name} takes a GDAREProblem, not {type(prob).__name__}; nothing was run on the device")
    try:
        beta, B, Rinv = prob.G
        gamma, Ct, S = prob.Q
    except (TypeError, ValueError):
        raise TypeError(f"{name}: G and Q must be lowrank(B, Rinv) and lowrank(Ct, S) objects; nothing was run on the device") from None
    Rinv, S = np.asarray(Rinv, dtype=float), np.asarray(S, dtype=float)
    m, q = np.shape(B)[-1], np.shape(Ct)[-1]
    Rs = None if beta == 1 and np.array_equal(Rinv, np.eye(m)) else beta * Rinv
    Ss = None if gamma == 1 and np.array_equal(S, np.eye(q)) else gamma * S
    return _gdare_check(name, prob.E, prob.A, B, Ct, Rs, Ss)


def _upload_all(ctx, mats):
    ups = [ctx.upload(M) if M is not None else None for M in mats]
    return ups, [u.ptr if u is not None else None for u in ups]


def _gdare_feedback(E, A, B, Ct, Rs, Ss, X):
    """K = R⁻¹Bᵀ X (I + GX)⁻¹ A"""
    RB = B.T if Rs is None else Rs @ B.T
    return RB @ X @ np.linalg.solve(np.eye(E.shape[0]) + B @ (RB @ X), A)


def solve_gdale_dense(prob: GDALEProblem, alg=None, dual=False, ctx=None, return_info=False):
    """solve(::GDALEProblem, ::Doubling): the dense X of AᵀXA − EᵀXE = −C (dual=True: A X Aᵀ − E X Eᵀ = −C) by the squared Smith iteration on
    E⁻¹A on the device (`dre_dense_stein_solve`): one Gauss-Jordan inversion, three GEMMs and one fused update per iteration.  E⁻¹A must have
    its eigenvalues inside the unit circle (DREError(-7) otherwise).  return_info: (X, dict(iters, step)).  Wrong types and shapes are errors
    before anything runs on the device."""
    name = "solve_gdale_dense"
    alg = Doubling() if alg is None else alg
    _doubling_check(name, alg)
    E, A, Cm = _gdale_operands(name, prob)
    ctx = ctx or dev.default_context()
    keep, ptrs = _upload_all(ctx, (E, A, Cm))
    xp = C.c_void_p()
    ii, dd = (C.c_int64 * 2)(), (C.c_double * 2)()
    maxiters, tol, _ = _sign_params(alg)
    ctx.chk(ctx.lib.dre_dense_stein_solve(ctx.ptr, *ptrs, 1 if dual else 0, maxiters, tol, C.byref(xp), ii, dd))
    X = dev.DenseMatrix(ctx, xp).numpy()
    del keep
    return (X, dict(iters=int(ii[0]), step=float(dd[0]))) if return_info else X


def gdale_residual_dense(prob: GDALEProblem, X, dual=False, ctx=None, return_info=False):
    """C + AᵀXA − EᵀXE (dual=True: C + A X Aᵀ − E X Eᵀ), symmetrised, on the device as an ndarray; return_info adds dict(norm, scaled) with
    the scaled norm ‖R‖_F / (‖C‖_F + ‖AᵀXA‖_F + ‖EᵀXE‖_F)."""
    E, A, Cm, Xh = _gdale_operands("gdale_residual_dense", prob, X)
    ctx = ctx or dev.default_context()
    keep, ptrs = _upload_all(ctx, (E, A, Cm, Xh))
    rp, nrm, sc = C.c_void_p(), C.c_double(), C.c_double()
    ctx.chk(ctx.lib.dre_dense_stein_residual(ctx.ptr, *ptrs, 1 if dual else 0, C.byref(rp), C.byref(nrm), C.byref(sc)))
    R = dev.DenseMatrix(ctx, rp).numpy()
    del keep
    return (R, dict(norm=nrm.value, scaled=sc.value)) if return_info else R


def solve_gdare_dense(prob: GDAREProblem, alg=None, ctx=None, return_info=False):
    """solve(::GDAREProblem, ::Doubling): the dense stabilizing solution X of Q + AᵀX(I + GX)⁻¹A − EᵀXE = 0 with G = β B R⁻¹ Bᵀ and
    Q = γ Cᵀ S C on the device (`dre_dense_dare_solve`): the structure-preserving doubling algorithm at order n and up to alg.max_refine
    Newton (Hewer) steps.  Open-loop unstable plants are fine as long as (A, B, E) is d-stabilizable and (A, C, E) d-detectable.
    return_info: (X, dict(iters, refinements, res0, res, K)) with the scaled residuals ‖R‖_F / (‖Q‖_F + ‖AᵀX(I + GX)⁻¹A‖_F + ‖EᵀXE‖_F) after
    the doubling and at the end, and the feedback K = R⁻¹Bᵀ X (I + GX)⁻¹ A (β folded in)."""
    name = "solve_gdare_dense"
    alg = Doubling() if alg is None else alg
    _doubling_check(name, alg)
    E, A, B, Ct, Rs, Ss = _gdare_operands(name, prob)
    ctx = ctx or dev.default_context()
    keep, (pE, pA, pB, pCt, pR, pS) = _upload_all(ctx, (E, A, B, Ct, Rs, Ss))
    xp = C.c_void_p()
    ii, dd = (C.c_int64 * 2)(), (C.c_double * 2)()
    maxiters, tol, max_refine = _sign_params(alg)
    ctx.chk(ctx.lib.dre_dense_dare_solve(ctx.ptr, pE, pA, pB, pR, pCt, pS, maxiters, tol, max_refine, C.byref(xp), ii, dd))
    X = dev.DenseMatrix(ctx, xp).numpy()
    del keep
    if return_info:
        return X, dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1]), K=_gdare_feedback(E, A, B, Ct, Rs, Ss, X))
    return X


def solve_gdare_pair(E, A, B, C_out, alg=None, Rinv=None, S=None, ctx=None, return_info=False):
    """Both Riccati equations of discrete-time LQG design from ONE doubling (`dre_dense_dare_solve_pair`) -> (X, Y):
        Q + AᵀX(I + GX)⁻¹A − EᵀXE = 0   (regulator)        G + A Y (I + QY)⁻¹ Aᵀ − E Y Eᵀ = 0   (filter)        G = B R⁻¹ Bᵀ, Q = Cᵀ S C
    (Rinv m x m and S q x q: None is the identity).  X is bit for bit what solve(GDAREProblem(E, A, G, Q), Doubling()) returns; Y is the limit
    of the G-sequence of the same doubling and needs no back-transformation.  return_info=True adds dict(iters, regulator=dict(iters,
    refinements, res0, res), filter=the same, K, L) with K = R⁻¹Bᵀ X (I + GX)⁻¹ A and the Kalman gain L = A Y (I + QY)⁻¹ Cᵀ S.  Wrong types
    and shapes are errors before anything runs on the device."""
    name = "solve_gdare_pair"
    alg = Doubling() if alg is None else alg
    _doubling_check(name, alg)
    Ch = _dense_f64(C_out)
    if Ch.ndim != 2:
        raise ValueError(f"{name}: C must be q x n, got {Ch.shape}; nothing was run on the device")
    Eh, Ah, Bh, Ct, Rh, Sh = _gdare_check(name, E, A, B, np.ascontiguousarray(Ch.T), Rinv, S)
    ctx = ctx or dev.default_context()
    keep, (pE, pA, pB, pCt, pR, pS) = _upload_all(ctx, (Eh, Ah, Bh, Ct, Rh, Sh))
    maxiters, tol, max_refine = _sign_params(alg)
    xp, yp = C.c_void_p(), C.c_void_p()
    ii, dd = (C.c_int64 * 4)(), (C.c_double * 4)()
    ctx.chk(ctx.lib.dre_dense_dare_solve_pair(ctx.ptr, pE, pA, pB, pR, pCt, pS, maxiters, tol, max_refine, C.byref(xp), C.byref(yp), ii, dd))
    X, Y = dev.DenseMatrix(ctx, xp).numpy(), dev.DenseMatrix(ctx, yp).numpy()
    del keep
    if not return_info:
        return X, Y
    SC = Ct.T if Sh is None else Sh @ Ct.T
    L = Ah @ Y @ np.linalg.solve(np.eye(Eh.shape[0]) + Ct @ (SC @ Y), Ct @ (np.eye(Ct.shape[1]) if Sh is None else Sh))
    info = dict(iters=int(ii[0]), regulator=dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1])),
                filter=dict(iters=int(ii[2]), refinements=int(ii[3]), res0=float(dd[2]), res=float(dd[3])),
                K=_gdare_feedback(Eh, Ah, Bh, Ct, Rh, Sh, X), L=L)
    return (X, Y), info


def gdare_residual_dense(prob: GDAREProblem, X, ctx=None, return_info=False):
    """Q + AᵀX(I + GX)⁻¹A − EᵀXE (symmetrised) on the device as an ndarray; return_info adds dict(norm, scaled) with the scaled norm of
    solve_gdare_dense."""
    name = "gdare_residual_dense"
    E, A, B, Ct, Rs, Ss = _gdare_operands(name, prob)
    Xh = _dense_f64(X)
    if Xh.shape != E.shape:
        raise ValueError(f"{name}: X must be {E.shape[0]} x {E.shape[0]}, got {Xh.shape}; nothing was run on the device")
    ctx = ctx or dev.default_context()
    keep, (pE, pA, pB, pCt, pR, pS, pX) = _upload_all(ctx, (E, A, B, Ct, Rs, Ss, Xh))
    rp, nrm, sc = C.c_void_p(), C.c_double(), C.c_double()
    ctx.chk(ctx.lib.dre_dense_dare_residual(ctx.ptr, pE, pA, pB, pR, pCt, pS, pX, C.byref(rp), C.byref(nrm), C.byref(sc)))
    R = dev.DenseMatrix(ctx, rp).numpy()
    del keep
    return (R, dict(norm=nrm.value, scaled=sc.value)) if return_info else R


# ------------------------------------------------------------------------------------------------
# The generalized Sylvester equation by the coupled sign iteration; H2 norm, inner product and error    (csrc/dense_sylvester.hip)
# ------------------------------------------------------------------------------------------------
@dataclass
class GSYLEProblem:
    """A X F + E X B = −C with A, E n x n, B, F m x m and C n x m; E=None or F=None is the identity.  Both pencils (A, E) and (B, F) must be
    c-stable."""
    E: Any
    A: Any
    F: Any
    B: Any
    C: Any


def _gsyle_pencils(name, E, A, F, B):
    """the checked dense f64 operands (E, F None for the identity) and the orders (n, m)"""
    A, B = _dense_f64(A), _dense_f64(B)
    if A.ndim != 2 or B.ndim != 2 or A.shape[0] < 1 or B.shape[0] < 1 or A.shape[0] != A.shape[1] or B.shape[0] != B.shape[1]:
        raise ValueError(f"{name}: A and B must be square of orders n, m >= 1, got {A.shape} and {B.shape}; nothing was run on the device")
    n, m = A.shape[0], B.shape[0]
    out = []
    for nm, M, k in (("E", E, n), ("F", F, m)):
        if M is not None:
            M = _dense_f64(M)
            if M.shape != (k, k):
                raise ValueError(f"{name}: {nm} must be {k} x {k} (or None for the identity), got {M.shape}; nothing was run on the device")
        out.append(M)
    return out[0], A, out[1], B, n, m


def _gsyle_rect(name, what, M, n, m):
    M = _dense_f64(M)
    if M.shape != (n, m):
        raise ValueError(f"{name}: {what} must be {n} x {m}, got {M.shape}; nothing was run on the device")
    return M


def _gsyle_operands(name, prob, X=None):
    if not isinstance(prob, GSYLEProblem):
        raise TypeError(f"{name} takes a GSYLEProblem, not {type(prob).__name__}; nothing was run on the device")
    E, A, F, B, n, m = _gsyle_pencils(name, prob.E, prob.A, prob.F, prob.B)
    mats = [E, A, F, B, _gsyle_rect(name, "C", prob.C, n, m)]
    if X is not None:
        mats.append(_gsyle_rect(name, "X", X, n, m))
    return mats


def _sign_check(name, alg):
    if not isinstance(alg, MatrixSign):
        raise TypeError(f"{name} takes alg = MatrixSign(), not {type(alg).__name__}; nothing was run on the device")
    maxiters, tol, max_refine = _sign_params(alg)
    if not 1 <= maxiters <= 1000 or max_refine < 0:
        raise ValueError(f"{name}: MatrixSign.maxiters must be in 1 .. 1000 and max_refine >= 0; nothing was run on the device")
    return maxiters, tol, max_refine


def _transposed_flag(name, transposed):
    if not isinstance(transposed, (bool, np.bool_)):
        raise TypeError(f"{name}: transposed must be a bool, not {type(transposed).__name__}; nothing was run on the device")
    return 1 if transposed else 0


def _sylvester_info(ii, dd):
    return dict(iters=int(ii[0]), refinements=int(ii[1]), res0=float(dd[0]), res=float(dd[1]), step=float(dd[2]))


def solve_gsyle_dense(prob: GSYLEProblem, alg=None, transposed=False, ctx=None, return_info=False):
    """solve(::GSYLEProblem, ::MatrixSign): the dense X of A X F + E X B = −C (transposed=True: AᵀX Fᵀ + EᵀX Bᵀ = −C) by the coupled sign
    iteration on the device (`dre_dense_sylvester_solve`): the two pencils iterate in lock-step under one scaling factor and the right-hand
    side rides along; up to alg.max_refine refinement steps replay the residual through the kept sequence.  A pencil that is not c-stable is
    DREError(-7) and the message names it.  return_info: (X, dict(iters, refinements, res0, res, step)) with the relative residuals
    ‖C + AXF + EXB‖_F / ‖C‖_F before and after the refinement and C's last relative step.  Wrong types and shapes are errors before anything
    runs on the device."""
    name = "solve_gsyle_dense"
    alg = MatrixSign() if alg is None else alg
    maxiters, tol, max_refine = _sign_check(name, alg)
    flag = _transposed_flag(name, transposed)
    mats = _gsyle_operands(name, prob)
    ctx = ctx or dev.default_context()
    keep, (pE, pA, pF, pB, pC) = _upload_all(ctx, mats)
    xp = C.c_void_p()
    ii, dd = (C.c_int64 * 2)(), (C.c_double * 3)()
    ctx.chk(ctx.lib.dre_dense_sylvester_solve(ctx.ptr, pE, pA, pF, pB, pC, flag, maxiters, tol, max_refine, C.byref(xp), ii, dd))
    X = dev.DenseMatrix(ctx, xp).numpy()
    del keep
    return (X, _sylvester_info(ii, dd)) if return_info else X


def gsyle_residual_dense(prob: GSYLEProblem, X, transposed=False, ctx=None, return_info=False):
    """C + A X F + E X B (transposed=True: C + AᵀX Fᵀ + EᵀX Bᵀ) on the device as an ndarray; return_info adds dict(norm, scaled) with the scaled
    norm ‖Res‖_F / (‖C‖_F + ‖AXF‖_F + ‖EXB‖_F)."""
    name = "gsyle_residual_dense"
    flag = _transposed_flag(name, transposed)
    mats = _gsyle_operands(name, prob, X)
    ctx = ctx or dev.default_context()
    keep, (pE, pA, pF, pB, pC, pX) = _upload_all(ctx, mats)
    rp, nrm, sc = C.c_void_p(), C.c_double(), C.c_double()
    ctx.chk(ctx.lib.dre_dense_sylvester_residual(ctx.ptr, pE, pA, pF, pB, pC, pX, flag, C.byref(rp), C.byref(nrm), C.byref(sc)))
    R = dev.DenseMatrix(ctx, rp).numpy()
    del keep
    return (R, dict(norm=nrm.value, scaled=sc.value)) if return_info else R


class SylvesterFactorization:
    """A kept coupled sign iteration of the two pencils (A, E) and (B, F) on the device (`dre_sylvester_create`), beside `SignFactorization`:
    every right-hand side of A X F + E X B = −C, in either direction, costs a replay only.  The operands are dense matrices or `DenseMatrix`
    objects already on the device; E=None or F=None is the identity.  A context manager; `close()` frees the device memory."""

    def __init__(self, E, A, F, B, maxiters=50, tol=None, ctx=None):
        name = "SylvesterFactorization"
        if not (isinstance(maxiters, (int, np.integer)) and 1 <= maxiters <= 1000):
            raise ValueError(f"{name}: maxiters must be an integer in 1 .. 1000, got {maxiters!r}; nothing was run on the device")
        if tol is not None and not (np.isfinite(tol) and tol > 0):
            raise ValueError(f"{name}: tol must be None or a positive number, got {tol!r}; nothing was run on the device")
        ops = dict(E=E, A=A, F=F, B=B)
        if not any(isinstance(M, dev.DenseMatrix) for M in ops.values()):
            ops["E"], ops["A"], ops["F"], ops["B"], _, _ = _gsyle_pencils(name, E, A, F, B)
        elif ops["A"] is None or ops["B"] is None:
            raise ValueError(f"{name}: A and B are required; nothing was run on the device")
        self.ctx = ctx or dev.default_context()
        d = {k: (M if M is None or isinstance(M, dev.DenseMatrix) else self.ctx.upload(_dense_f64(M))) for k, M in ops.items()}
        self.n, self.m = d["A"].shape[0], d["B"].shape[0]
        p = C.c_void_p()
        self.ctx.chk(self.ctx.lib.dre_sylvester_create(self.ctx.ptr, d["E"].ptr if d["E"] is not None else None, d["A"].ptr,
                                                       d["F"].ptr if d["F"] is not None else None, d["B"].ptr, int(maxiters),
                                                       float(tol) if tol is not None else 0.0, C.byref(p)))
        self.ptr = p
        self._fin = weakref.finalize(self, self.ctx.lib.dre_sylvester_destroy, self.ctx.ptr, p)
        it = C.c_int64()
        self.ctx.lib.dre_sylvester_iters(p, C.byref(it))
        self.iters = int(it.value)

    def close(self):
        self._fin()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def solve(self, Cm, transposed=False, download=True, max_refine=2):
        """A X F + E X B = −C (transposed=True: AᵀX Fᵀ + EᵀX Bᵀ = −C) for an n x m C (ndarray or `DenseMatrix`) -> (X, info); download=False
        leaves X on the device.  The untransposed X is bit for bit what solve(GSYLEProblem, MatrixSign()) returns."""
        name = "SylvesterFactorization.solve"
        flag = _transposed_flag(name, transposed)
        if not (isinstance(max_refine, (int, np.integer)) and max_refine >= 0):
            raise ValueError(f"{name}: max_refine must be an integer >= 0, got {max_refine!r}; nothing was run on the device")
        if isinstance(Cm, dev.DenseMatrix):
            if Cm.shape != (self.n, self.m):
                raise ValueError(f"{name}: C must be {self.n} x {self.m}, got {Cm.shape}; nothing was run on the device")
            Cd = Cm
        else:
            Cd = self.ctx.upload(_gsyle_rect(name, "C", Cm, self.n, self.m))
        xp = C.c_void_p()
        ii, dd = (C.c_int64 * 2)(), (C.c_double * 3)()
        self.ctx.chk(self.ctx.lib.dre_sylvester_solve(self.ctx.ptr, self.ptr, Cd.ptr, flag, int(max_refine), C.byref(xp), ii, dd))
        X = dev.DenseMatrix(self.ctx, xp)
        return (X.numpy() if download else X), _sylvester_info(ii, dd)


def _h2_system(name, what, sys_):
    """the checked dense operands (E, A, B, C) of one system; E None is the identity"""
    try:
        E, A, B, Cm = sys_
    except (TypeError, ValueError):
        raise TypeError(f"{name}: {what} must be a tuple (E, A, B, C); nothing was run on the device") from None
    mats = []
    for nm, M in (("E", E), ("A", A), ("B", B), ("C", Cm)):
        if M is None and nm == "E":
            mats.append(None)
            continue
        if not isinstance(M, (np.ndarray, LowRankUpdate, ScaledPencil)) and not sp.issparse(M):
            raise TypeError(f"{name}: {nm} of {what} must be a matrix, not {type(M).__name__}; nothing was run on the device")
        mats.append(np.asarray(_dense_operator(M), dtype=float))
    Eh, Ah, Bh, Ch = mats
    n = Ah.shape[0] if Ah.ndim == 2 else 0
    if Eh is None:
        Eh = np.eye(n)
    if n < 1 or Ah.shape != (n, n) or Eh.shape != (n, n) or Bh.ndim != 2 or Bh.shape[0] != n or Ch.ndim != 2 or Ch.shape[1] != n:
        raise ValueError(f"{name}: E and A of {what} must be n x n, B n x m and C q x n; got {Eh.shape}, {Ah.shape}, {Bh.shape}, {Ch.shape}; "
                         "nothing was run on the device")
    return Eh, Ah, Bh, Ch


def _h2_ports(name, s1, s2):
    if (s1[2].shape[1], s1[3].shape[0]) != (s2[2].shape[1], s2[3].shape[0]):
        raise ValueError(f"{name}: the two systems have (m, q) = {(s1[2].shape[1], s1[3].shape[0])} and {(s2[2].shape[1], s2[3].shape[0])}; "
                         "nothing was run on the device")


def _gsyle_residual_device(ctx, Ed, Ad, Fd, Bd, Cd, Xd):
    """C + A X F + E X B of operands on the device, left there"""
    rp = C.c_void_p()
    ctx.chk(ctx.lib.dre_dense_sylvester_residual(ctx.ptr, Ed.ptr, Ad.ptr, Fd.ptr, Bd.ptr, Cd.ptr, Xd.ptr, 0, C.byref(rp), None, None))
    return dev.DenseMatrix(ctx, rp)


def _h2_trace(ctx, Cl, X, dX, Cr):
    """tr(Cl (X + dX) Crᵀ) from two q x q blocks: the products run on the device, the blocks are added on the host"""
    return float(sum(np.trace(ctx.gemm(False, True, 1.0, ctx.gemm(False, False, 1.0, Cl, M), Cr).numpy()) for M in (X, dX)))


# The H2 formulas cancel, so their traces are wanted to rounding level, eps tr, while a solve stops refining at a relative residual of
# 100 n eps (measured on SteelProfile(371): the Gramian's residual 2e-12, its trace off by 13 eps tr).  Each trace therefore gets the first-order
# correction tr(Cl dX Crᵀ), where dX is ONE replay of the solution's residual through the kept sequence: the refinement step the solver's own
# rule does not take, applied to the trace alone.
def _h2_norm2(name, system, alg, ctx, side=""):
    """‖H‖²_H2 = tr(C P Cᵀ), A P Eᵀ + E P Aᵀ = −B Bᵀ: one sign factorisation, the dual replay of B Bᵀ and of the residual; q x q blocks come back"""
    Eh, Ah, Bh, Ch = system
    maxiters, tol, max_refine = _sign_params(alg)
    Ed, Ad, Bd, Cd = (ctx.upload(M) for M in (Eh, Ah, Bh, Ch))
    try:
        sign = SignFactorization(Ed, Ad, maxiters, tol if tol > 0 else None, ctx)
    except DREError as e:
        if e.code == -7 and side:
            raise DREError(-7, f"{name}: the {side} is not c-stable ({e})") from None
        raise
    try:
        R = ctx.gemm(False, True, 1.0, Bd, Bd)
        P, _ = sign.solve_dense(R, max_refine, download=False, transposed=True)
        Res = _gsyle_residual_device(ctx, Ed, Ad, ctx.upload(np.ascontiguousarray(Eh.T)), ctx.upload(np.ascontiguousarray(Ah.T)), R, P)
        dP, _ = sign.solve_dense(Res, 0, download=False, transposed=True)
    finally:
        sign.close()
    return _h2_trace(ctx, Cd, P, dP, Cd)


def _h2_inner(name, s1, s2, alg, ctx, side=""):
    """⟨H₁, H₂⟩ = tr(C₁ X C₂ᵀ), A₁ X E₂ᵀ + E₁ X A₂ᵀ = −B₁ B₂ᵀ: one Sylvester factorisation with the right pencil (A₂ᵀ, E₂ᵀ), the replay of B₁ B₂ᵀ
    and of the residual"""
    (E1, A1, B1, C1), (E2, A2, B2, C2) = s1, s2
    maxiters, tol, max_refine = _sign_params(alg)
    E1d, A1d, B1d, C1d, B2d, C2d = (ctx.upload(M) for M in (E1, A1, B1, C1, B2, C2))
    E2t, A2t = ctx.upload(np.ascontiguousarray(E2.T)), ctx.upload(np.ascontiguousarray(A2.T))
    try:
        fac = SylvesterFactorization(E1d, A1d, E2t, A2t, maxiters, tol if tol > 0 else None, ctx)
    except DREError as e:
        if e.code == -7 and side and "right pencil" in str(e):
            raise DREError(-7, f"{name}: the {side} is not c-stable ({e})") from None
        raise
    with fac:
        R = ctx.gemm(False, True, 1.0, B1d, B2d)
        X, _ = fac.solve(R, download=False, max_refine=max_refine)
        dX, _ = fac.solve(_gsyle_residual_device(ctx, E1d, A1d, E2t, A2t, R, X), download=False, max_refine=0)
    return _h2_trace(ctx, C1d, X, dX, C2d)


def h2_norm(E, A, B, C, alg=MatrixSign(), ctx=None):
    """‖H‖_H2 = √tr(C P Cᵀ) of E ẋ = A x + B u, y = C x (c-stable pencil (A, E); E=None: the identity), where A P Eᵀ + E P Aᵀ = −B Bᵀ: one sign
    factorisation on the Lyapunov path (`SignFactorization.solve_dense(..., transposed=True)`), one replay of the Gramian's residual, whose trace
    is added as a first-order correction, and the products on the device; only q x q blocks come back to the host.  DREError(-7) for a pencil that is not c-stable."""
    name = "h2_norm"
    _sign_check(name, alg)
    system = _h2_system(name, "the system", (E, A, B, C))
    return math.sqrt(max(_h2_norm2(name, system, alg, ctx or dev.default_context()), 0.0))


def h2_inner(sys1, sys2, alg=MatrixSign(), ctx=None):
    """The H2 inner product ⟨H₁, H₂⟩ = tr(C₁ X C₂ᵀ) of two systems (E, A, B, C) with the same numbers of inputs and outputs, where
    A₁ X E₂ᵀ + E₁ X A₂ᵀ = −B₁ B₂ᵀ: one Sylvester solve (`SylvesterFactorization`) with the right pencil (A₂ᵀ, E₂ᵀ) on the device; only a q x q
    block comes back.  DREError(-7) names the pencil that is not c-stable."""
    name = "h2_inner"
    _sign_check(name, alg)
    s1, s2 = _h2_system(name, "sys1", sys1), _h2_system(name, "sys2", sys2)
    _h2_ports(name, s1, s2)
    return _h2_inner(name, s1, s2, alg, ctx or dev.default_context())


def h2_error(E, A, B, C, rom, return_info=False, alg=MatrixSign(), ctx=None):
    """‖H − H_r‖_H2 of the full system against a `ReducedModel` or `LQGReducedModel` (or a tuple (Er, Ar, Br, Cr)) by the closed formula
        err² = ‖H‖² − 2 ⟨H, H_r⟩ + ‖H_r‖²
    from `h2_norm` twice and `h2_inner` once, all on the device.  The formula cancels: its absolute accuracy is of the order
    floor = eps (‖H‖² + ‖H_r‖²), so an error below √eps ‖H‖ cannot be resolved and err² may come out slightly negative; the function returns
    √max(err², 0).  return_info adds dict(err2, norm2, norm2_r, inner, floor).  A reduced model that is not c-stable (an `LQGReducedModel` of
    an unstable plant, for instance) is DREError(-7) and names the reduced side."""
    name = "h2_error"
    _sign_check(name, alg)
    if isinstance(rom, (ReducedModel, LQGReducedModel)):
        rsys = (rom.Er, rom.Ar, rom.Br, rom.Cr)
    elif isinstance(rom, tuple) and len(rom) == 4:
        rsys = rom
    else:
        raise TypeError(f"{name}: rom must be a ReducedModel, an LQGReducedModel or a tuple (Er, Ar, Br, Cr), not {type(rom).__name__}; "
                        "nothing was run on the device")
    full, red = _h2_system(name, "the system", (E, A, B, C)), _h2_system(name, "the reduced model", rsys)
    _h2_ports(name, full, red)
    ctx = ctx or dev.default_context()
    norm2_r = _h2_norm2(name, red, alg, ctx, side="reduced model")
    norm2 = _h2_norm2(name, full, alg, ctx)
    inner = _h2_inner(name, full, red, alg, ctx, side="reduced model")
    err2 = norm2 - 2.0 * inner + norm2_r
    err = math.sqrt(max(err2, 0.0))
    if return_info:
        return err, dict(err2=err2, norm2=norm2, norm2_r=norm2_r, inner=inner, floor=float(np.finfo(float).eps) * (norm2 + norm2_r))
    return err


def _rom_h2_error(self, E, A, B, C, **kw):
    """‖H − H_r‖_H2 of the full system (E, A, B, C) against this reduced model: `h2_error` with its keyword arguments"""
    return h2_error(E, A, B, C, self, **kw)


ReducedModel.h2_error = _rom_h2_error
LQGReducedModel.h2_error = _rom_h2_error


def solve(prob, alg, **kw):
    """CommonSolve.solve for the problems of this path."""
    if isinstance(prob, GDREProblem):
        return solve_gdre(prob, alg, **kw)
    if isinstance(prob, GALEProblem):
        if isinstance(alg, MatrixSign):
            return solve_gale_dense(prob, alg, **kw)
        if isinstance(alg, FactoredSign):
            return solve_gale_factored_sign(prob, alg, **kw)
        return solve_gmres(prob, alg, **kw) if isinstance(alg, GMRES) else solve_gale(prob, alg, **kw)
    if isinstance(prob, GAREProblem):
        if isinstance(alg, MatrixSign):
            return solve_gare_dense(prob, alg, **kw)
        return solve_gare(prob, alg, **kw)
    if isinstance(prob, GDALEProblem):
        return solve_gdale_dense(prob, alg, **kw)
    if isinstance(prob, GDAREProblem):
        return solve_gdare_dense(prob, alg, **kw)
    if isinstance(prob, GSYLEProblem):
        return solve_gsyle_dense(prob, alg, **kw)
    raise TypeError(f"unsupported problem type {type(prob).__name__}")
