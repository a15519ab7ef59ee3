"""ctypes glue for dre_sym_eig_probe (include/dre_hip.h): one run of the Householder + QL chain with every intermediate result as NumPy arrays."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import dre_amd as D

ERR_INVALID = -1
_dead = []          # the message of the first call that failed with anything but DRE_ERR_INVALID: nothing more is started on the device after it


def _chk(ctx, call):
    if _dead:
        raise RuntimeError("an earlier call failed on the device, no further call is made: " + _dead[0])
    try:
        ctx.chk(call())
    except D.DREError as e:
        if e.code != ERR_INVALID:
            _dead.append(str(e))
        raise


def probe(ctx, S, tolfac=4.0, want_eig=True, abs_tol=-1.0, floor_mode=0, deflate=1e-3, ids=None, want_v=True):
    """SimpleNamespace(jdim, nref, q, snorm, d, e, tau, V, w, Z, B); w, Z are None without want_eig or at jdim = 0, B is None without ids,
    V is None without want_v (the handle is not even asked for).  ids: a list, or "all" for every column 0 .. jdim - 1.  S may be an array or a DenseMatrix already on the device."""
    Sd = S if isinstance(S, D.DenseMatrix) else ctx.upload(S)
    ii = (C.c_int64 * 3)()
    snorm = C.c_double()
    h = [C.c_void_p() for _ in range(7)]
    idv, nids = None, 0
    if isinstance(ids, str):
        assert ids == "all"
        nids = -1          # every column 0 .. jdim - 1
    elif ids is not None:
        idv = np.ascontiguousarray(ids, dtype=np.int32)
        nids = len(idv)
    refs = [C.byref(p) for p in h]
    if not want_v:
        refs[3] = None
    _chk(ctx, lambda: ctx.lib.dre_sym_eig_probe(ctx.ptr, Sd.ptr, float(tolfac), int(bool(want_eig)), float(abs_tol), int(floor_mode), float(deflate),
                                                idv.ctypes.data_as(C.POINTER(C.c_int32)) if idv is not None and len(idv) else None,
                                                nids, ii, C.byref(snorm), *refs))
    arr = [D.DenseMatrix(ctx, p).numpy() if p.value else None for p in h]
    d, e, tau, V, w, Z, B = arr
    return SimpleNamespace(jdim=int(ii[0]), nref=int(ii[1]), q=int(ii[2]), snorm=snorm.value, d=d.ravel(), e=e.ravel(), tau=tau.ravel(), V=V,
                           w=None if w is None else w.ravel(), Z=Z, B=B)


def public(ctx, S, tolfac=4.0):
    """dre_sym_eig: (w ascending, vectors q x j)"""
    Sd = S if isinstance(S, D.DenseMatrix) else ctx.upload(S)
    w, v = C.c_void_p(), C.c_void_p()
    _chk(ctx, lambda: ctx.lib.dre_sym_eig(ctx.ptr, Sd.ptr, float(tolfac), C.byref(w), C.byref(v)))
    return D.DenseMatrix(ctx, w).numpy().ravel(), D.DenseMatrix(ctx, v).numpy()
