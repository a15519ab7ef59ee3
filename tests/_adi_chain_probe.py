"""ctypes glue for dre_adi_chain_probe (include/dre_hip.h): one run of the dense-inverse ADI chain on NumPy operands, every buffer back as an array."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import dre_amd as D
import _adi_chain_model as M

ERR_INVALID = -1
FAST, GROUP, BUILD = 0, 1, 2
_dead = []          # the message of the first call that failed with anything but DRE_ERR_INVALID: nothing more is started on the device after it


def _f(a):
    return None if a is None else np.asfortranarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data


def make_args(kind, n, k, stacks, *, m=0, wks=None, wks_null=None, cycle=None, mu=(-1.0,), R0=None, T=None, g=0, nit=1, base_it=0, maxiters=1 << 20,
              tdiag=0, mode=-1, nt=-1, ld=None, alpha=1.0, abstol=0.0, outputs=True):
    """(AdiChainProbeArgsC, keep-alive namespace with the output arrays).  stacks / wks: lists of matrices."""
    keep = SimpleNamespace()
    nstack = len(stacks)
    keep.stacks = np.concatenate([_f(s).ravel(order="F") for s in stacks]) if nstack else None
    keep.wks = np.concatenate([_f(w).ravel(order="F") for w in wks]) if wks else None
    keep.wks_null = None if wks_null is None else np.ascontiguousarray(wks_null, dtype=np.int32)
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    keep.mu = mu
    keep.cycle = np.ascontiguousarray(range(len(mu)) if cycle is None else cycle, dtype=np.int32)
    keep.R0 = None if R0 is None else _f(R0).ravel(order="F")
    keep.T = None if T is None else _f(T).ravel(order="F")
    ld = n + 2 if ld is None else ld
    ct = (max(k, 1) + 15) // 16
    blocks = 2 * g if kind == GROUP else 2
    ok = outputs and n >= 1 and 1 <= k <= 512 and 1 <= nit <= 480 and ld >= 1 and nstack >= 1
    if ok and kind != BUILD:
        keep.V = np.empty(ld * k * (nit + 1)); keep.R = np.empty(ld * k * (nit + 1))
        keep.Rp = np.empty(M.rpack_doubles(n, k) * (nit + 1))
        keep.G = np.empty(k * k * 2 * (g if kind == GROUP else 1))
    else:
        keep.V = keep.R = keep.Rp = keep.G = None
    keep.packs = np.empty(nstack * blocks * M.nstrip(n) * M.kst(n) * 64) if (outputs and n >= 1 and nstack >= 1 and blocks >= 2) else None
    keep.state_i = np.full(4, -99, dtype=np.int32)
    keep.state_d = np.full(2 + M.RING, -99.0)
    a = D._lib.AdiChainProbeArgsC(kind=kind, n=n, m=m, k=k, nstack=nstack, ncyc=len(mu), g=g, nit=nit, base_it=base_it, maxiters=maxiters, tdiag=tdiag,
                                  mode=mode, nt=nt, ld=ld, alpha=alpha, abstol=abstol,
                                  stacks=_ptr(keep.stacks), wks=_ptr(keep.wks), wks_null=_ptr(keep.wks_null), cycle=_ptr(keep.cycle), mu=_ptr(keep.mu),
                                  R0=_ptr(keep.R0), T=_ptr(keep.T), V=_ptr(keep.V), R=_ptr(keep.R), packs=_ptr(keep.packs), Rp=_ptr(keep.Rp), G=_ptr(keep.G),
                                  state_i=_ptr(keep.state_i), state_d=_ptr(keep.state_d))
    keep.ld, keep.ct, keep.blocks = ld, ct, blocks
    return a, keep


def probe(ctx, kind, n, k, stacks, **kw):
    """One run.  SimpleNamespace: packs (nstack x flat), and for the chains V, R (ld x k x (nit + 1) as [slot][ld, k] views), Rp (nit + 1 slots), G,
    iters, done, res_norm, abstol, norms (512), mode, nt."""
    if _dead:
        raise RuntimeError("an earlier call failed on the device, no further call is made: " + _dead[0])
    a, keep = make_args(kind, n, k, stacks, **kw)
    try:
        ctx.chk(ctx.lib.dre_adi_chain_probe(ctx.ptr, C.byref(a)))
    except D.DREError as e:
        if e.code != ERR_INVALID:
            _dead.append(str(e))
        raise
    out = SimpleNamespace(packs=keep.packs.reshape(len(stacks), -1))
    if kind == BUILD:
        return out
    nit, ld = a.nit, keep.ld
    out.V = keep.V.reshape(nit + 1, k, ld).transpose(0, 2, 1)          # [slot][row, col]
    out.R = keep.R.reshape(nit + 1, k, ld).transpose(0, 2, 1)
    out.Rp = keep.Rp.reshape(nit + 1, -1)
    out.G = keep.G.reshape(-1, k, k).transpose(0, 2, 1)
    out.iters, out.done, out.mode, out.nt = (int(v) for v in keep.state_i)
    out.res_norm, out.abstol, out.norms = float(keep.state_d[0]), float(keep.state_d[1]), keep.state_d[2:].copy()
    return out
