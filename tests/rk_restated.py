"""Fixed-grid explicit Runge-Kutta, restated for the tests: the tableaus written out as exact fractions (independently of
covomix_amd.acoustic.TABLEAUS), the evaluation times of a solve in numpy fp32, and a generic integrator in torch that works in any
dtype and skips zero weights the way the stage kernel does."""
from fractions import Fraction as Fr

import numpy as np
import torch

# name -> (a: strictly lower-triangular rows, b, c, nominal order)
TABLEAUS = {
    "euler": ((), (Fr(1),), (Fr(0),), 1),
    "midpoint": (((Fr(1, 2),),), (Fr(0), Fr(1)), (Fr(0), Fr(1, 2)), 2),
    "heun2": (((Fr(1),),), (Fr(1, 2), Fr(1, 2)), (Fr(0), Fr(1)), 2),
    "heun3": (((Fr(1, 3),), (Fr(0), Fr(2, 3))), (Fr(1, 4), Fr(0), Fr(3, 4)), (Fr(0), Fr(1, 3), Fr(2, 3)), 3),
    # the 3/8 rule: what torchdiffeq's fixed-grid "rk4" runs
    "rk4": (((Fr(1, 3),), (Fr(-1, 3), Fr(1)), (Fr(1), Fr(-1), Fr(1))), (Fr(1, 8), Fr(3, 8), Fr(3, 8), Fr(1, 8)),
            (Fr(0), Fr(1, 3), Fr(2, 3), Fr(1)), 4),
    "rk4_classic": (((Fr(1, 2),), (Fr(0), Fr(1, 2)), (Fr(0), Fr(0), Fr(1))), (Fr(1, 6), Fr(1, 3), Fr(1, 3), Fr(1, 6)),
                    (Fr(0), Fr(1, 2), Fr(1, 2), Fr(1)), 4),
}


def as_floats(name):
    """(a, b, c) of a restated tableau as python floats"""
    a, b, c, _ = TABLEAUS[name]
    return tuple(tuple(float(x) for x in row) for row in a), tuple(float(x) for x in b), tuple(float(x) for x in c)


def grid_f32(steps):
    """torchdiffeq's fixed grid for step_size = 1 / steps on [0, 1], in fp32"""
    g = np.arange(steps + 1, dtype=np.float32) * np.float32(1.0 / steps)
    g[-1] = np.float32(1.0)
    return g


def evaluation_times(steps, name):
    """(one fp32 time per field evaluation, dt per step) of `steps` steps: t0 + fp32(c_j) dt, the grid point t1 for c_j = 1"""
    _, _, c = as_floats(name)
    g = grid_f32(steps)
    times, dts = [], []
    for t0, t1 in zip(g[:-1], g[1:]):
        dt = np.float32(t1 - t0)
        dts.append(float(dt))
        for cj in c:
            t = t0 if cj == 0.0 else (t1 if cj == 1.0 else np.float32(t0 + np.float32(np.float32(cj) * dt)))
            times.append(float(t))
    return times, dts


def odeint_rk(fn, y0, grid, a, b, c):
    """y(grid[-1]) of dy/dt = fn(t, y) from y(grid[0]) = y0: one explicit Runge-Kutta step (a, b, c) per grid interval.  Stage j is
    evaluated at t0 + c_j dt (the grid point itself when c_j = 1) on y + sum_i (dt a_ji) k_i; a weight that is 0 is skipped."""
    rows = ((),) + tuple(a) + (tuple(b),)
    n = len(b)
    y = y0
    for t0, t1 in zip(grid[:-1], grid[1:]):
        dt = t1 - t0
        k = []
        for j in range(n + 1):
            x = y
            for i, w in enumerate(rows[j]):
                if w != 0:
                    x = x + k[i] * (dt * w)
            if j == n:
                y = x
                break
            t = t0 if c[j] == 0 else (t1 if c[j] == 1 else t0 + c[j] * dt)
            k.append(fn(t, x))
    return y
