"""The host restatement of round 3 (morbit.jl_amd/sampling.py: _rbf_round3, RbfModel.jl:269-307) against cases derived by hand from the
reference's text, and the phase-I driver on host databases (prepare_update_models, RbfModel.jl:518-655) on a scripted run whose
metas are written out literally.  No GPU: the small filters stay on the host and round 4 finds the model full (max_model_points = d + 1)."""
import numpy as np
import pytest

from morbit.jl_amd import database, descent, sampling
from morbit.jl_amd.rbf_model import RbfConfig

E = np.eye(2)


def r3(x, lb, ub, piv, dirs, max_new=10, n_missing=None, efl=False, force=False):
    return sampling._rbf_round3(None, np.array(lb, float), np.array(ub, float), np.array(x, float), piv, dirs,
                                max_new, len(dirs) if n_missing is None else n_missing, efl, force)


def test_free_box():
    # e0: steps -1 (lb) and +1 (ub), |+1| >= |-1| picks +1; (0, .5): steps -2 and +2, picks +2
    pts, fl, rem = r3([0, 0], [-1, -1], [1, 1], 0.1, [np.array([1.0, 0.0]), np.array([0.0, 0.5])])
    assert pts.tolist() == [[1.0, 0.0], [0.0, 1.0]] and fl is True and rem == []


def test_iterate_on_a_bound():
    # x0 = ub0 along +e0: the ub entry is 0 (on the bound, pointing out), the lb entry -2; |0| >= |-2| fails: len = -2
    pts, fl, rem = r3([1, 0], [-1, -1], [1, 1], 0.1, [E[0]])
    assert pts.tolist() == [[-1.0, 0.0]] and fl is True and rem == []
    # along -e0 the ub entry is Inf, the lb entry (-1 - 1) / -1 = 2: sigma+ = 2
    pts, _, _ = r3([1, 0], [-1, -1], [1, 1], 0.1, [-E[0]])
    assert pts.tolist() == [[-1.0, 0.0]]


FIXED = dict(x=[0.5, 0.25], lb=[0.5, 0.0], ub=[0.5, 1.0], piv=0.05)


def test_fixed_coordinate_fails_the_pivot_test():
    # lb0 = ub0 = x0, direction e0: entries Inf (lb, pointing in) and 0 (ub, pointing out): sigma+ = 0, no negative entry: len 0
    assert descent.intersect_box(np.array(FIXED["x"]), E[0], np.array(FIXED["lb"]), np.array(FIXED["ub"])) == 0.0
    pts, fl, rem = r3(dirs=[E[0], E[1]], **FIXED)
    assert pts.tolist() == [[0.5, 0.25], [0.5, 1.0]] and fl is False and rem == []      # kept, not fully linear; e1: -.25 / +.75


def test_fixed_coordinate_with_ensure_fully_linear_asks_for_the_rebuild():
    assert r3(dirs=[E[1], E[0]], efl=True, **FIXED) == (None, None, None)


def test_fixed_coordinate_with_force_rebuild_is_kept():
    pts, fl, rem = r3(dirs=[E[0], E[1]], efl=True, force=True, **FIXED)
    assert pts.tolist() == [[0.5, 0.25], [0.5, 1.0]] and fl is False and rem == []


def test_max_new():
    dirs = [E[0], E[1]]
    pts, fl, rem = r3([0, 0], [-1, -1], [1, 1], 0.1, dirs, max_new=0)
    assert pts.shape == (0, 2) and fl is False and [v.tolist() for v in rem] == [[1, 0], [0, 1]]
    pts, fl, rem = r3([0, 0], [-1, -1], [1, 1], 0.1, dirs, max_new=1)
    assert pts.tolist() == [[1.0, 0.0]] and fl is False and [v.tolist() for v in rem] == [[0, 1]]
    pts, fl, rem = r3([0, 0], [-1, -1], [1, 1], 0.1, dirs, max_new=-3)
    assert pts.shape == (0, 2) and fl is False and len(rem) == 2
    with pytest.raises(AssertionError):
        r3([0, 0], [-1, -1], [1, 1], 0.1, dirs, n_missing=3)


def test_component_in_a_fixed_coordinate():
    # x = (0, .5, .25), dir = (.6, .8, 0): coordinate 0 is fixed and contributes Inf (lb) and 0 (ub), coordinate 1 the steps
    # (.4 - .5) / .8 and (.6 - .5) / .8, coordinate 2 nothing.  sigma+ = min(Inf, 0, ~.125) = 0, sigma- = ~-.125, and |0| >= |-.125|
    # fails: the reference's len is the NEGATIVE step, about -0.125, although the direction leaves the box at once
    x, dr, lb, ub = np.array([0, .5, .25]), np.array([.6, .8, 0]), np.array([0, .4, .15]), np.array([0, .6, .35])
    want = (0.4 - 0.5) / 0.8
    assert abs(want + 0.125) < 1e-15
    assert descent.intersect_box(x, dr, lb, ub) == want
    pts, fl, _ = sampling._rbf_round3(None, lb, ub, x, 0.01, [dr], 5, 1, True, False)
    assert pts.tolist() == [[0 + want * .6, .5 + want * .8, .25]] and fl is True


def test_zero_direction_gives_a_nan_row_and_does_not_fail():
    pts, fl, _ = r3([0, 0], [-1, -1], [1, 1], 0.1, [np.zeros(2)], efl=True)
    assert np.isnan(pts).all() and fl is True


def test_round3_many_rebuilds_in_place():
    res = sampling.rbf_round3_many([np.array(FIXED["lb"])] * 2, [np.array(FIXED["ub"])] * 2, [np.array(FIXED["x"])] * 2, 0.05,
                                   [[E[1], E[0]], None], 10, 2, ensure_fully_linear=[True, False])
    a, b = res
    assert a.rebuilt and a.new_points.tolist() == [[0.5, 0.25], [0.5, 1.0]] and a.fully_linear is False and a.remaining_directions == []
    assert not b.rebuilt and b.new_points.tolist() == [[0.5, 0.25], [0.5, 1.0]] and b.fully_linear is False


def test_reversed_order_takes_the_last_direction_first():
    Z = np.array([[1.0, 0.0], [0.0, 0.5]])            # rows are directions
    (r,) = sampling.rbf_round3_many([[-1, -1]], [[1, 1]], [[0, 0]], 0.1, [Z], 1, 1, reversed_order=True)
    assert r.new_points.tolist() == [[0.0, 1.0]] and [v.tolist() for v in r.remaining_directions] == [[1.0, 0.0]]


def test_prepare_update_models_many_scripted_run():
    """d = 3 with the third coordinate fixed by the global bounds (lb = ub = .5), three iterations of one start.  Every number is a
    power of two, so the geometry below is exact."""
    cfg = RbfConfig(max_model_points=4)                # theta_enlarge 2 / 2, theta_pivot 1/4; round 4 finds the model full
    lb, ub, delta_max = np.array([0, 0, .5]), np.array([1, 1, .5]), 0.5
    db = database.HostDatabase(3, 1)
    db.append(np.array([[.5, .5, .5]]), np.array([[0.0]]))
    run = lambda x_index, delta, efl: sampling.prepare_update_models(cfg, [db], [db.sites[x_index].copy()], [x_index], delta, delta_max,
                                                                           lb, ub, ensure_fully_linear=efl)[0]
    strip = lambda m: {k: (v if k != "improving_directions" else [np.asarray(u).tolist() for u in v]) for k, v in m.items()}

    # 1: an empty database around x.  Round 1 finds nothing, its directions are e2, e1, e0; e2 lies in the fixed coordinate: len 0, the
    # pivot test fails and, with ensure_fully_linear, the start is rebuilt along e0, e1, e2 (box [.25, .75]^2: the steps are -.25 / +.25,
    # the tie picks +.25); the e2 point is x itself and fails again: not fully linear
    m = run(0, 0.125, True)
    assert strip(m) == dict(center_index=0, round1_indices=[], round2_indices=[], round3_indices=[1, 2, 3], round4_indices=[],
                            fully_linear=False, improving_directions=[], rebuilt=True)
    assert db.sites[1:].tolist() == [[.75, .5, .5], [.5, .75, .5], [.5, .5, .5]] and np.isnan(db.values[1:]).all()
    db.set_values([1, 2, 3], np.zeros((3, 1)))

    # 2: x = row 1, no ensure_fully_linear.  Box 1 holds rows 0, 2, 3 (shifted (-.25, 0, 0), (-.25, .25, 0), (-.25, 0, 0)): the
    # filter takes 0 (first of the largest), then 2 (its part orthogonal to e0 is (0, .25, 0)); row 3 repeats row 0.  One site is
    # missing, round 2 runs (Delta is not Delta_max) and finds nothing new, round 3 samples along +-e2: len 0, kept, not fully linear
    m = run(1, 0.125, False)
    assert strip(m) == dict(center_index=1, round1_indices=[0, 2], round2_indices=[], round3_indices=[4], round4_indices=[],
                            fully_linear=False, improving_directions=[], rebuilt=False)
    assert db.sites[4].tolist() == [.75, .5, .5]
    db.set_values([4], np.zeros((1, 1)))

    # 3: x = row 2 with ensure_fully_linear, Delta_1 = .5: box [0, 1] x [.25, 1].  Round 1 takes 0 and 1, round 3's only direction is
    # +-e2 and fails: rebuild.  e0: -.5 / +.5 -> +.5; e1: (.25 - .75) = -.5 / (1 - .75) = +.25 -> -.5; e2: x itself
    m = run(2, 0.25, True)
    assert strip(m) == dict(center_index=2, round1_indices=[], round2_indices=[], round3_indices=[5, 6, 7], round4_indices=[],
                            fully_linear=False, improving_directions=[], rebuilt=True)
    assert db.sites[5:].tolist() == [[1.0, .75, .5], [.5, .25, .5], [.5, .75, .5]]
