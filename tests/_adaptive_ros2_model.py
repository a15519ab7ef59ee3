"""Host NumPy model of the device's adaptive dense Ros2 driver (csrc/dense_adaptive.hip) on the oracle's `lyap_dense`: one step of
`solve_dense_ros2` restated so that it returns the embedded error estimate, and the step-size controller, decision for decision.

One trial step of size tau = |h| from (t, X), with K = B'XE and gF = gamma tau (A - BK) - E/2 (gamma = 1 + 1/sqrt 2):

    K1   = lyap(gF, E, sym(C'C + A'XE + E'XA - K'K))
    K2   = lyap(gF, E, sym(-tau^2 (B'K1E)'(B'K1E) - (2 - 1/gamma) E'K1E)) + (4 - 1/gamma) K1
    Xnew = X + (tau/2) K2,     D = Xnew - (X + tau K1)              (X + tau K1: the embedded first-order solution)
    err  = sqrt(mean_ij (D_ij / sc_ij)^2),   sc_ij = atol + rtol max(|X_ij|, |Xnew_ij|)

Controller: accept iff err <= 1; fac = clamp(0.9 err^(-1/2), 0.2, 5), 5 for err == 0, 0.2 (and a rejection) for a non-finite err, at most 1 on
the trial right after a rejection; the next |h| is tau * fac clamped to [dt_min, dt_max].  tf and the tstops are hit exactly: with d the distance
to the next of them, the step is d when d <= 1.1 |h| and d/2 when d < 2 |h|; on arrival t is set to that value itself.  A rejection at a
step <= dt_min and more than max_steps trials are failures (`StepFailure`, the device's DRE_ERR_STEP).
"""
import math

import numpy as np

import dre_oracle as o

GAMMA = 1.0 + 1.0 / math.sqrt(2.0)
FAC_MIN, FAC_MAX, SAFETY = 0.2, 5.0, 0.9


class StepFailure(Exception):
    pass


def ros2_step(E, A, B, CtC, X, tau):
    """(Xnew, D) of one Ros2 step of size tau > 0 (oracle/dre_oracle.py, solve_dense_ros2, one pass of its loop)"""
    K = (B.T @ X) @ E
    gF = GAMMA * tau * (A - B @ K) - E / 2.0
    AtXE = (A.T @ X) @ E
    R = CtC + AtXE + AtXE.T - K.T @ K
    R = 0.5 * (R + R.T)
    K1 = o.lyap_dense(gF, E, R)
    BtK1E = (B.T @ K1) @ E
    R2 = (-tau ** 2 * BtK1E).T @ BtK1E - (2.0 - 1.0 / GAMMA) * (E.T @ K1 @ E)
    R2 = 0.5 * (R2 + R2.T)
    K2 = o.lyap_dense(gF, E, R2) + (4.0 - 1.0 / GAMMA) * K1
    Xnew = X + (tau / 2.0) * K2
    return Xnew, Xnew - (X + tau * K1)


def error_measure(D, X, Xnew, rtol, atol):
    sc = atol + rtol * np.maximum(np.abs(X), np.abs(Xnew))
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.mean((D / sc) ** 2)))


def decide(err):
    """(accept, fac) of one trial, before the cap after a rejection"""
    if not math.isfinite(err):
        return False, FAC_MIN
    if err == 0.0:
        return True, FAC_MAX
    return err <= 1.0, min(FAC_MAX, max(FAC_MIN, SAFETY / math.sqrt(err)))


def check_arguments(t0, tf, dt0, rtol, atol, dt_min, dt_max, max_steps, tstops):
    if not (tf != t0 and dt0 != 0.0 and (dt0 > 0) == (tf > t0)):
        raise ValueError("dt0 must be nonzero and of the sign of tf - t0")
    if not (rtol > 0 and atol > 0 and 0 <= dt_min <= dt_max and max_steps >= 1):
        raise ValueError("rtol > 0, atol > 0, 0 <= dt_min <= dt_max, max_steps >= 1 expected")
    prev = t0
    for s in tstops:
        if not ((prev < s < tf) if tf > t0 else (prev > s > tf)):
            raise ValueError("tstops must lie strictly between t0 and tf, strictly monotone in the direction of integration")
        prev = s


class Trajectory:
    """t, X (every accepted state), K, err per accepted step; trials: (t, tau, err, accepted) of every trial step"""

    def __init__(self):
        self.t, self.X, self.K, self.err, self.trials = [], [], [], [], []
        self.accepted = self.rejected = 0


def solve(E, A, B, C, X0, tspan, dt0, rtol=1e-3, atol=1e-6, dt_min=0.0, dt_max=math.inf, max_steps=10_000, tstops=(), step=None):
    """The adaptive driver.  `step(X, tau) -> (Xnew, D)` replaces the Ros2 step (tests of the controller alone)."""
    t0, tf = float(tspan[0]), float(tspan[1])
    check_arguments(t0, tf, dt0, rtol, atol, dt_min, dt_max, max_steps, tstops)
    E, A = np.asarray(E, dtype=float), np.asarray(A, dtype=float)
    CtC = C.T @ C
    if step is None:
        step = lambda X, tau: ros2_step(E, A, B, CtC, X, tau)
    dirn = 1.0 if tf > t0 else -1.0
    clamp = lambda h: min(max(h, dt_min), dt_max)
    stops = [float(s) for s in tstops] + [tf]
    out = Trajectory()
    X, t, h = np.asarray(X0, dtype=float), t0, clamp(abs(dt0))
    out.t.append(t); out.X.append(X); out.K.append((B.T @ X) @ E)
    nxt, after_reject, trials = 0, False, 0
    while nxt < len(stops):
        d = abs(stops[nxt] - t)
        tau, hit = h, False
        if d <= 1.1 * h:
            tau, hit = d, True
        elif d < 2.0 * h:
            tau = 0.5 * d
        trials += 1
        if trials > max_steps:
            raise StepFailure(f"more than max_steps = {max_steps} trial steps (t = {t})")
        Xnew, D = step(X, tau)
        err = error_measure(D, X, Xnew, rtol, atol)
        accept, fac = decide(err)
        if after_reject:
            fac = min(fac, 1.0)
        out.trials.append((t, tau, err, accept))
        if accept:
            t = stops[nxt] if hit else t + dirn * tau
            if hit:
                nxt += 1
            X = Xnew
            out.accepted += 1
            out.t.append(t); out.X.append(X); out.K.append((B.T @ X) @ E); out.err.append(err)
            after_reject = False
        else:
            if tau <= dt_min:
                raise StepFailure(f"step rejected at dt_min = {dt_min} (t = {t}, err = {err})")
            out.rejected += 1
            after_reject = True
        h = clamp(tau * fac)
    out.t = np.array(out.t); out.err = np.array(out.err)
    return out


def fixed_ros2(E, A, B, C, X0, T, nsteps):
    """nsteps Ros2 steps of size T / nsteps (the accuracy reference of the tests)"""
    CtC = C.T @ C
    X = np.asarray(X0, dtype=float)
    for _ in range(nsteps):
        X, _ = ros2_step(E, A, B, CtC, X, T / nsteps)
    return X


def stabilizing_solution(E, A, B, C):
    """The stabilizing solution of C'C + A'XE + E'XA - E'XBB'XE = 0: a long coarse Ros2 run from X = 0 (L-stable, it lands near the fixed point
    with a c-stable closed loop), then Newton-Kleinman steps on `lyap_dense` to rounding level"""
    CtC = C.T @ C
    X = fixed_ros2(E, A, B, C, np.zeros_like(E), 5000.0, 100)
    for _ in range(30):
        K = (B.T @ X) @ E
        Xn = o.lyap_dense(A - B @ K, E, CtC + K.T @ K)
        done = np.linalg.norm(Xn - X) <= 1e-14 * np.linalg.norm(Xn)
        X = Xn
        if done:
            break
    return X


def predicted_steps_at_rest(T, dt0, dt_max):
    """Accepted steps of a run in which every trial is accepted with fac = 5 (a start at the stabilizing GARE solution): the count of the
    must-hit rule alone, for a span of length T without tstops"""
    t, h, count = 0.0, min(abs(dt0), dt_max), 0
    while True:
        d = abs(T - t)
        count += 1
        if d <= 1.1 * h:
            return count
        tau = 0.5 * d if d < 2.0 * h else h
        t, h = t + tau, min(5.0 * tau, dt_max)


def stiff_pencil(n, m=2, q=3, seed=0):
    """Seeded random pencil with a stiff spectrum: A = -diag(logspace(-2, 1.5, n)) + 0.1 randn, E symmetric positive definite near I.  The random
    part can push the slowest open-loop modes a little over the axis (max Re lambda(E^-1 A) = 0.30 at n = 33, seed 2, and 0.33 at n = 70, seed 0):
    the stage pencil gamma tau A - E/2 at X = 0 is c-stable for tau < 1 / (2 gamma max Re lambda), about 0.9 there"""
    rng = np.random.default_rng(seed)
    A = -np.diag(np.logspace(-2, 1.5, n)) + 0.1 * rng.standard_normal((n, n))
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    E = E @ E.T
    return E, A, rng.standard_normal((n, m)), rng.standard_normal((q, n))
