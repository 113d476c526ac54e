"""Time grids, embedded pairs and the grid fitter, restated for the tests independently of covomix_amd.acoustic: the named grids in
numpy fp64 rounded to fp32, the lower-order weights as exact fractions, an integrator that returns the estimate of every step, the
fitter in numpy, and the analytic problem with a sharp feature that the fitter is tested on."""
import math
from fractions import Fraction as Fr

import numpy as np
import torch

import rk_restated as rr

# name -> (b_err, order of the lower-order solution); euler has none
B_ERR = {
    "midpoint": ((Fr(1), Fr(0)), 1),
    "heun2": ((Fr(1), Fr(0)), 1),
    "heun3": ((Fr(0), Fr(1, 2), Fr(1, 2)), 2),
    "rk4": ((Fr(0), Fr(1, 2), Fr(1, 2), Fr(0)), 2),
    "rk4_classic": ((Fr(0), Fr(1), Fr(0), Fr(0)), 2),
}
SWAY_MAX = 2.0 / (math.pi - 2.0)


def named_grid(spec, steps):
    """'uniform', 'cosine' or 'sway:<s>' as an fp32 numpy array"""
    if spec == "uniform":
        return rr.grid_f32(steps)
    u = np.arange(steps + 1, dtype=np.float64) / steps
    if spec == "cosine":
        t = (1.0 - np.cos(np.pi * u)) / 2.0
    else:
        s = float(spec.split(":")[1])
        t = u + s * (np.cos(np.pi * u / 2.0) - 1.0 + u)
    t[0], t[-1] = 0.0, 1.0
    return t.astype(np.float32)


def evaluation_times(grid, name):
    """rk_restated.evaluation_times on any fp32 grid"""
    _, _, c = rr.as_floats(name)
    g = np.asarray(grid, dtype=np.float32)
    times, dts = [], []
    for t0, t1 in zip(g[:-1], g[1:]):
        dt = np.float32(t1 - t0)
        dts.append(float(dt))
        for cj in c:
            t = t0 if cj == 0.0 else (t1 if cj == 1.0 else np.float32(t0 + np.float32(np.float32(cj) * dt)))
            times.append(float(t))
    return times, dts


def odeint_rk_err(fn, y0, grid, a, b, c, b_err):
    """rk_restated.odeint_rk that also returns, per step, delta = sum_j k_j (dt (b_j - b_err_j)) (zero weights skipped, j order) and the
    state after the step"""
    rows = ((),) + tuple(a) + (tuple(b),)
    n = len(b)
    y, deltas, states = y0, [], []
    for t0, t1 in zip(grid[:-1], grid[1:]):
        dt = t1 - t0
        k = []
        for j in range(n):
            x = y
            for i, w in enumerate(rows[j]):
                if w != 0:
                    x = x + k[i] * (dt * w)
            t = t0 if c[j] == 0 else (t1 if c[j] == 1 else t0 + c[j] * dt)
            k.append(fn(t, x))
        d = None
        for j in range(n):
            w = b[j] - b_err[j]
            if w != 0:
                d = k[j] * (dt * w) if d is None else d + k[j] * (dt * w)
        for j in range(n):
            if b[j] != 0:
                y = y + k[j] * (dt * b[j])
        deltas.append(d)
        states.append(y)
    return y, deltas, states


def fit(E, grid, q, steps):
    """error-equidistributing grid: density E_k^(1/(q+1)) / h_k on step k, the new points at equal parts of its integral"""
    grid = np.asarray(grid, dtype=np.float64)
    F = np.concatenate([[0.0], np.cumsum(np.maximum(np.asarray(E, dtype=np.float64), 1e-300) ** (1.0 / (q + 1)))])
    g = np.interp(np.linspace(0.0, F[-1], steps + 1), F, grid)
    g[0], g[-1] = 0.0, 1.0
    return g.astype(np.float32)


# ---- y' = w(t) (-y2, y1), w = 1 + 40 exp(-((t - 0.85) / 0.05)^2), y(0) = (1, 0): the rotation by the integral of w
def sharp_field(t, y):
    w = 1.0 + 40.0 * math.exp(-((float(t) - 0.85) / 0.05) ** 2)
    return torch.stack([-w * y[1], w * y[0]])


def sharp_exact():
    th = 1.0 + 40.0 * 0.05 * math.sqrt(math.pi) / 2.0 * (math.erf((1.0 - 0.85) / 0.05) - math.erf((0.0 - 0.85) / 0.05))
    return torch.tensor([math.cos(th), math.sin(th)], dtype=torch.float64)
