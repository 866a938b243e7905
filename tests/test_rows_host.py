"""The per-row placement solver without a GPU: the float64 mirror of the algorithm (``tests/_rows_reference.py``)
against scipy's BFGS on every row alone, and the keywords that select the solver."""
import inspect

import numpy as np
import pytest

import _rows_reference as ref
from pymde_amd import dense

LOSSES = {"quadratic": ref.quadratic, "huber": ref.huber(1.0)}


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("loss", sorted(LOSSES))
def test_mirror_reaches_what_scipy_bfgs_reaches_on_every_row_alone(loss, d):
    """Seed-31 inputs, eps = 1e-5, at most 300 sweeps: every row ends converged or stalled, with f_i <= scipy's
    per-row BFGS minimum (gtol 1e-8) + 1e-4 f_i(start).  (Cubic has rows in different local minima at d = 2, worst
    excess 1e-2 of the starting value, and is left out.)"""
    _, _, X_old, start, D = ref.seed31_problem(d)
    fun = ref.row_objective(LOSSES[loss], X_old, D)
    state, sweeps, evaluations = ref.solve(fun, start, eps=1e-5, max_iter=300)
    best, first = ref.scipy_row_minima(fun, start)
    excess = (state.f - best) / first
    print(f"{loss} d={d}: sweeps {sweeps}, evaluations {evaluations:.1f}, counts {state.counts()}, "
          f"worst excess {excess.max():.3g}")
    assert sweeps <= 300
    assert set(np.unique(state.status)) <= {ref.CONVERGED, ref.STALLED}
    assert (state.f <= best + 1e-4 * first).all()
    assert evaluations < sweeps + 1          # finished rows are no longer evaluated


def test_float32_state_follows_the_float64_state():
    """The mirror with the kernel's float32 state reaches the float64 run's values to float32 resolution."""
    _, _, X_old, start, D = ref.seed31_problem(2)
    fun = ref.row_objective(ref.quadratic, X_old, D)
    s64, _, _ = ref.solve(fun, start, eps=1e-5, max_iter=300)
    s32, _, _ = ref.solve(fun, start, eps=1e-5, max_iter=300, state_dtype=np.float32)
    assert set(np.unique(s32.status)) <= {ref.CONVERGED, ref.STALLED}
    np.testing.assert_allclose(s32.f, s64.f, rtol=1e-6)


def test_unknown_solver_is_a_value_error_before_any_device_work():
    placement = dense.DensePlacement.__new__(dense.DensePlacement)      # no device behind it
    with pytest.raises(ValueError, match="'joint'.*'rows'.*bogus"):
        placement.embed(solver="bogus")
    landmark = dense.LandmarkMDE.__new__(dense.LandmarkMDE)
    with pytest.raises(ValueError, match="placement_solver.*bogus"):
        landmark.embed(placement_solver="bogus")


def test_solver_keywords_are_in_the_signatures():
    embed = inspect.signature(dense.DensePlacement.embed).parameters
    assert embed["solver"].default == "joint"
    assert inspect.signature(dense.LandmarkMDE.embed).parameters["placement_solver"].default == "joint"
    assert "solver" not in inspect.signature(dense.DensePlacement.__init__).parameters
