"""The row-per-lane schedule of the close's 6x6 solve (csrc/icp/solve_lanes.h), restated in numpy with its operation
order, against the oracle's one-lane sequence: byte for byte on every system the GPU test uses.  No GPU: an ordering
mistake in the schedule shows here, before a card is involved."""
import os

import numpy as np
import pytest

import _lane_solve_cases as cases
import _surface_fit_ref as sf


@pytest.fixture(scope="module")
def sys_():
    return cases.systems()


def test_the_systems_take_every_pivot_choice_and_zero_pivots(sys_):
    A, b, n_finite = sys_
    assert A.shape == (2004, 6, 6) and b.shape == (2004, 6) and n_finite == 2002
    pairs, zeros = cases.coverage(A, b, 2000)
    assert pairs == {(k, p) for k in range(6) for p in range(k, 6)} and len(pairs) == 21
    assert zeros >= 1
    assert np.isfinite(A[:n_finite]).all() and not np.isfinite(A[n_finite]).all() and not np.isfinite(A[n_finite + 1]).all()


def test_lane_schedule_equals_the_oracle_byte_for_byte(sys_, oracle):
    A, b, n_finite = sys_
    for s in range(len(A)):
        x, ok, tr, _ = cases.solve6_lanes_ref(A[s], b[s])
        ok_o, x_o = oracle.solve6(A[s], b[s])
        assert ok == bool(ok_o), s
        if s < n_finite:
            assert ok and np.array_equal(cases.raw(x), cases.raw(np.asarray(x_o, np.float64))), s
            x_r, ok_r = sf.solve6_ldlt(A[s], b[s])
            assert ok_r and np.array_equal(cases.raw(x_r), cases.raw(np.asarray(x_o, np.float64))), s
    # ties keep the identity permutation; the zero matrix solves to zero
    x, ok, tr, zp = cases.solve6_lanes_ref(A[2000], b[2000])
    assert tr == list(range(6)) and ok and np.array_equal(x, b[2000] / 3.0)
    x, ok, tr, zp = cases.solve6_lanes_ref(A[2001], b[2001])
    assert ok and zp and not x.any()
    assert not cases.solve6_lanes_ref(A[2002], b[2002])[1] and not cases.solve6_lanes_ref(A[2003], b[2003])[1]


def test_the_switch_decides_the_path_and_defaults_to_the_lane_solve():
    """PEDP_ICP_LANE_SOLVE=0 and PEDP_ICP_SERIAL_CLOSE=1 keep the one-lane solve; unset, the lane solve is in force."""
    from pedp_hip import _lib

    on = ("head_close", "cert", "steady")
    kw = dict(n_source=1000, n_target=5000, radius=1.0, resident=True)
    assert _lib.icp_path(on, lane_solve=1, **kw)["lane_solve"] is True
    assert _lib.icp_path(on, lane_solve=0, **kw)["lane_solve"] is False
    assert _lib.icp_path(on + ("serial_close",), lane_solve=1, **kw)["lane_solve"] is False
    assert _lib.icp_path(on, lane_solve=1, **dict(kw, radius=0.0))["lane_solve"] is False   # (not fused: no close of this kind)
    assert "lane_solve" not in _lib.icp_path(on, **kw)
    if not any(k in os.environ for k in ("PEDP_ICP_LANE_SOLVE", "PEDP_ICP_SERIAL_CLOSE")):
        assert _lib.icp_path(None, lane_solve=1, **kw)["lane_solve"] is True
