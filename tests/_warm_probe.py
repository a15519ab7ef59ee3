"""ctypes glue for dre_warm_probe (include/dre_hip.h): one entry point of csrc/warm.hip on NumPy operands, every output back as an array."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import dre_amd as D
import _warm_model as M

ERR_INVALID = -1
PROJECT, Z, ZAPPLY, SMALL, EIG, FINISH, CHAIN = range(7)
_dead = []          # the message of the first call that failed with anything but DRE_ERR_INVALID: nothing more is started on the device after it
_INPUTS = ("Q", "Yf", "Pf", "Z1", "Cw", "Res", "Cc", "parts", "S", "Wk", "Yp", "Pp", "tols_in", "basis")


def _flat(a):
    return None if a is None else np.asfortranarray(a, dtype=np.float64).ravel(order="F").copy()


def _ptr(a):
    return None if a is None else a.ctypes.data


def make_args(stage, *, n=0, q=0, m=0, kl=0, qn=0, mode=0, ldpad=0, reltol=0.0, abstol=-1.0, frac=1.0, budget_frac=0.4, outputs=True, **inputs):
    """(WarmProbeArgsC, keep-alive namespace with the output arrays and their shapes)"""
    keep = SimpleNamespace(shapes={})
    for name in _INPUTS:
        setattr(keep, name, _flat(inputs.pop(name, None)))
    assert not inputs, f"unknown arguments {sorted(inputs)}"
    nparts = 0 if keep.parts is None else keep.parts.size
    ld = n + ldpad
    mb = q + 16 if stage == CHAIN else m
    nstrip = (n + 15) // 16 if n >= 1 else 0
    shapes = {}
    if stage == PROJECT:
        shapes = dict(Z1_out=(ld, 16), Cw_out=(16, 16), slab=(256, M.project_slabs(n) if n >= 1 else 0))
    elif stage in (Z, ZAPPLY):
        shapes = dict(Zb=(ld, 16), Zy=(ld, 16))
        if stage == Z:
            shapes["W2"] = (ld, 16)
    elif stage == SMALL:
        shapes = dict(tols=(12, 1), Uc=(m, qn), T=(kl, kl), Cp=(m, 16))
        if mode == 1:
            shapes.update(Mout=(m, m), LTout=(m, m))
    elif stage == EIG:
        shapes = dict(U=(m, m))
    elif stage == FINISH:
        shapes = dict(R=(ld, 16 * ((kl + 15) // 16)), tols=(12, 1), slab=(nstrip, 1))
    elif stage == CHAIN:
        shapes = dict(R=(ld, qn), basis_out=(ld, 32 + q + 16), T=(kl, kl), tols=(12, 1), Uc=(mb, qn), Cp=(mb, 16))
    fields = {}
    if outputs:
        for name, shp in shapes.items():
            arr = np.full(max(shp[0] * shp[1], 1), -99.0)
            setattr(keep, "o_" + name, arr)
            fields[name] = _ptr(arr)
        keep.shapes = shapes
    keep.ticket = np.full(2, -99, dtype=np.int32)
    a = D._lib.WarmProbeArgsC(stage=stage, n=n, q=q, m=m, kl=kl, qn=qn, nparts=nparts, mode=mode, ldpad=ldpad, reserved=0, reltol=reltol, abstol=abstol,
                              frac=frac, budget_frac=budget_frac, ticket=_ptr(keep.ticket), **{k: _ptr(getattr(keep, k)) for k in _INPUTS}, **fields)
    return a, keep


def probe(ctx, stage, **kw):
    """One call.  SimpleNamespace with every output of the stage as a matrix (tols and FINISH's slab as vectors, PROJECT's slab as (nslab, 16, 16) with
    [b][i, j] the share of entry (i, j)), and ticket (2 ints)."""
    if _dead:
        raise RuntimeError("an earlier call failed on the device, no further call is made: " + _dead[0])
    a, keep = make_args(stage, **kw)
    try:
        ctx.chk(ctx.lib.dre_warm_probe(ctx.ptr, C.byref(a)))
    except D.DREError as e:
        if e.code != ERR_INVALID:
            _dead.append(str(e))
        raise
    out = SimpleNamespace(ticket=[int(v) for v in keep.ticket])
    for name, shp in keep.shapes.items():
        arr = getattr(keep, "o_" + name)[:shp[0] * shp[1]].reshape(shp, order="F")
        if shp[1] == 1:
            arr = arr[:, 0]
        if stage == PROJECT and name == "slab":
            arr = arr.T.reshape(-1, 16, 16).transpose(0, 2, 1)          # share (i, j) of workgroup b sits at 256 b + i + 16 j
        setattr(out, name, arr.copy())
    return out
