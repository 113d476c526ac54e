"""The fixed-grid Runge-Kutta solvers of the acoustic solve, host side (no GPU): the built-in tableaus against the order conditions
in exact arithmetic and against an ODE with a known order of convergence, the evaluation times against the numpy restatement bit
for bit, the restated integrator (tests/rk_restated.py) against the oracle's midpoint / Euler, and the stage kernel's descriptors."""
import math
from fractions import Fraction as Fr

import pytest
import torch

import rk_restated as rr
from covomix_amd.acoustic import TABLEAUS, Tableau, evaluation_times, resolve_method

NAMES = ("euler", "midpoint", "heun2", "heun3", "rk4", "rk4_classic")
ORDERS = dict(zip(NAMES, (1, 2, 2, 3, 4, 4)))


def test_built_ins_are_the_restated_tableaus():
    assert tuple(TABLEAUS) == NAMES == tuple(rr.TABLEAUS)
    for name in NAMES:
        a, b, c = rr.as_floats(name)
        t = TABLEAUS[name]
        assert (t.name, t.a, t.b, t.c) == (name, a, b, c), name
        assert t.stages == len(b) <= 4 and resolve_method(name) is t and resolve_method(t) is t
        assert hash(t) == hash(Tableau(name, a, b, c)) and t == Tableau(name, a, b, c)


@pytest.mark.parametrize("name", NAMES)
def test_order_conditions_in_exact_arithmetic(name):
    """Butcher's conditions up to the nominal order, on the fractions: order 1 sum b = 1 (and c = row sums of a); order 2 b.c = 1/2;
    order 3 b.c^2 = 1/3, b.(A c) = 1/6; order 4 b.c^3 = 1/4, sum b_i c_i a_ij c_j = 1/8, b.(A c^2) = 1/12, b.(A A c) = 1/24."""
    a, b, c, order = rr.TABLEAUS[name]
    assert order == ORDERS[name]
    n = len(b)
    A = [[a[i - 1][j] if 0 < i and j < i else Fr(0) for j in range(n)] for i in range(n)]
    assert len(c) == n and len(a) == n - 1 and all(len(row) == i + 1 for i, row in enumerate(a))
    dot = lambda u, v: sum((x * y for x, y in zip(u, v)), Fr(0))
    mat = lambda v: [dot(A[i], v) for i in range(n)]
    assert sum(b, Fr(0)) == 1
    assert list(c) == mat([Fr(1)] * n)
    c2, c3 = [x * x for x in c], [x ** 3 for x in c]
    conditions = {2: [(dot(b, c), Fr(1, 2))],
                  3: [(dot(b, c2), Fr(1, 3)), (dot(b, mat(c)), Fr(1, 6))],
                  4: [(dot(b, c3), Fr(1, 4)), (dot([x * y for x, y in zip(b, c)], mat(c)), Fr(1, 8)), (dot(b, mat(c2)), Fr(1, 12)),
                      (dot(b, mat(mat(c))), Fr(1, 24))]}
    for p in range(2, order + 1):
        for got, want in conditions[p]:
            assert got == want, (name, p, got, want)
    if order < 4:                                     # ... and not the next order's: the nominal order is the true one
        assert any(got != want for got, want in conditions[order + 1]), name


def _field(t, y):
    return -y * y + torch.sin(3.0 * t)


def _solve(steps, a, b, c):
    grid = torch.linspace(0.0, 1.0, steps + 1, dtype=torch.float64)
    return rr.odeint_rk(_field, torch.tensor([1.0, 0.3], dtype=torch.float64), grid, a, b, c)


@pytest.fixture(scope="module")
def reference_solution():
    return _solve(4096, *rr.as_floats("rk4_classic"))


@pytest.mark.parametrize("name", NAMES)
def test_observed_order_on_a_scalar_ode(name, reference_solution):
    """y' = -y^2 + sin 3t, y(0) = (1, 0.3), fp64: log2 of the error ratio from 16 to 32 steps with the PACKAGE's tableau lies within
    0.35 of the nominal order (measured when this was written: 0.99, 2.25, 2.02, 3.13, 3.99, 4.00).  Reference: 4096 classic RK4
    steps (error ~1e-15, five orders below the smallest error measured here)."""
    t = TABLEAUS[name]
    e16 = float((_solve(16, t.a, t.b, t.c) - reference_solution).norm())
    e32 = float((_solve(32, t.a, t.b, t.c) - reference_solution).norm())
    observed = math.log2(e16 / e32)
    print(f"FIGURE {name}: error at 16 steps {e16:.3e}, at 32 steps {e32:.3e}, observed order {observed:.2f}")
    assert abs(observed - ORDERS[name]) < 0.35, (name, observed)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("steps", [1, 2, 16])
def test_evaluation_times_equal_the_restatement_bit_for_bit(name, steps):
    n = TABLEAUS[name].stages
    want_t, want_dt = rr.evaluation_times(steps, name)
    for method in (name, TABLEAUS[name]):
        times, dts = evaluation_times(steps * n, method)
        assert times.dtype == torch.float32 and times.tolist() == want_t and dts == want_dt, (name, steps)
    assert len(want_t) == steps * n and abs(sum(want_dt) - 1.0) < 1e-6
    if TABLEAUS[name].c[-1] == 1.0:                   # a stage at c = 1 sits on the grid point itself: the last one on t = 1 exactly
        assert want_t[-1] == 1.0


def test_evaluation_times_refuse_what_they_cannot_run():
    for nfe, method in ((6, "rk4"), (3, "rk4"), (0, "rk4"), (7, "midpoint"), (4, "heun3"), (2, "heun3"), (0, "euler"), (-2, "midpoint")):
        with pytest.raises(ValueError):
            evaluation_times(nfe, method)
    for name in ("rk5", "RK4", "", "dopri5", None, 4):      # an unknown name used to run Euler without a word
        with pytest.raises(ValueError):
            evaluation_times(8, name)
        with pytest.raises(ValueError):
            resolve_method(name)


@pytest.mark.parametrize("a,b,c", [
    (((0.5,),), (0.5, 0.4), (0.0, 0.5)),                                   # sum b != 1
    (((0.5,),), (0.0, 1.0), (0.0, 0.4)),                                   # c is not the row sum
    (((0.5,),), (0.0, 1.0), (0.1, 0.5)),                                   # c_0 != 0
    (((0.5, 0.0),), (0.0, 1.0), (0.0, 0.5)),                               # a row too long (not strictly lower-triangular)
    ((), (0.0, 1.0), (0.0, 0.5)),                                          # a row missing
    (((0.5,),), (0.0, 1.0), (0.0, 0.5, 1.0)),                              # c too long
    ((), (), ()),                                                          # no stage
    (((0.25,), (0.0, 0.25), (0.0, 0.0, 0.25), (0.0, 0.0, 0.0, 0.25)), (0.2,) * 5, (0.0, 0.25, 0.25, 0.25, 0.25)),   # five stages
    (((float("nan"),),), (0.0, 1.0), (0.0, float("nan"))),
    ((("x",),), (0.0, 1.0), (0.0, 0.5)),
])
def test_a_bad_tableau_is_refused(a, b, c):
    with pytest.raises(ValueError):
        Tableau("bad", a, b, c)


def test_a_custom_tableau_is_accepted_everywhere_a_name_is():
    ralston = Tableau("ralston", ((2 / 3,),), (0.25, 0.75), (0.0, 2 / 3))
    times, dts = evaluation_times(4, ralston)
    assert len(times) == 4 and dts == [0.5, 0.5]
    assert {ralston: 1}[Tableau("ralston", [[2 / 3]], [0.25, 0.75], [0, 2 / 3])] == 1          # lists are frozen into tuples: hashable
    with pytest.raises(Exception):
        ralston.b = (1.0, 0.0)


@pytest.mark.parametrize("name,steps", [("midpoint", 7), ("euler", 11)])
def test_restated_integrator_agrees_with_the_oracle(name, steps):
    import covomix_oracle as orc
    grid = torch.linspace(0.0, 1.0, steps + 1, dtype=torch.float64)
    y0 = torch.tensor([1.0, 0.3, -0.7], dtype=torch.float64)
    want = orc.odeint_fixed(_field, y0, grid, name)
    got = rr.odeint_rk(_field, y0, grid, *rr.as_floats(name))
    assert float((got - want).abs().max()) <= 1e-12


def test_model_and_cli_validate_the_method_before_anything_runs():
    import covomix_amd.synthetic as syn
    from covomix_amd.conditional_model import CoVoMixModel
    from covomix_amd.generation import build_parser, run
    shapes = syn.acoustic_param_shapes(dim=128, dim_cond=160, dim_emb=64, depth=2, heads=2, streams=2)
    sd = {k: torch.from_numpy(v) for k, v in syn.synth_state_dict(shapes).items()}
    assert CoVoMixModel.from_state_dict(sd, ode_method="rk4", nfe=8).ode_method == "rk4"
    with pytest.raises(ValueError):
        CoVoMixModel.from_state_dict(sd, ode_method="rk5")
    args = build_parser().parse_args([])
    assert args.ode_method == "midpoint" and args.nfe == 32
    for argv in (["--ode_method", "rk4", "--nfe", "30"], ["--ode_method", "nope"]):
        with pytest.raises(ValueError):
            run(False, argv)


def test_stage_kernel_code_objects_use_no_scratch():
    """Both instances of the stage kernel (16-byte and 4-byte accesses) in the built library: no private segment, no LDS."""
    from covomix_amd import _lib
    from test_attention_form_d import _gfx950_kernel_descriptors
    kds = {k: v for k, v in _gfx950_kernel_descriptors(_lib.LIB_PATH).items() if "rk_stage_kernel" in k}
    assert len(kds) == 2, sorted(kds)
    for name, (group, private, vgprs) in kds.items():
        print(f"FIGURE {name}: LDS {group}, private segment {private}, VGPRs allocated {vgprs}")
        assert private == 0 and group == 0, (name, group, private)
