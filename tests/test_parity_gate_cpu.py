"""The yardstick of the normal equations without a GPU: the long-double truth the gate measures against (Oracle.eval_normal_truth_batch) and the gate
itself (tests/parity_gate.py), which must fail a device that is further from the truth than the double oracle allows, and the cap on how many
candidates of a launch may lean on the block-by-block explanation."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity_gate  # noqa: E402


def test_the_oracle_has_an_80_bit_long_double(ob):
    assert ob.ldbl_mant_dig() >= 64, "long double has %d mantissa bits: the 'truth' would be one more double evaluation" % ob.ldbl_mant_dig()
    ob.require_long_double()


@pytest.fixture(scope="module")
def small(synth, abi, ob):
    prob, meta = synth.make_scene(n_frames=4, pts_per_frame=2000, n_keypoints=600, seed=13)
    p = abi.reference_yaml_params()
    xs = synth.perturb(meta["x_gt"], np.random.default_rng(13), n=3)
    o = ob.Oracle(prob)
    yield p, xs, o
    o.close()


def test_the_batched_truth_is_the_per_candidate_truth(small, ob):
    p, xs, o = small
    plain = o.eval_normal(p, xs, nthreads=1)   # (one thread: its sums in a fixed order)
    batch = o.eval_normal_truth_batch(p, xs, nthreads=4)
    assert len(batch) == len(xs)
    for x, t, d in zip(xs, batch, plain):
        one = o.eval_normal_truth(p, x)[0]
        assert np.array_equal(t.H_np(), one.H_np()) and np.array_equal(t.b_np(), one.b_np())
        assert t.cost == one.cost and t.chi2 == one.chi2 and t.counts() == one.counts()
        # the truth is near the double evaluation (a broken mode switch would put it anywhere) but not the double evaluation itself
        assert t.counts() == d.counts() and d.n_factor_3d2d > 100
        for a, b in ((t.H_np(), d.H_np()), (t.b_np(), d.b_np())):
            big, small_ = parity_gate.worst_rel(b, a)
            assert big <= 1e-7 and small_ <= 1e-7, (big, small_)
        assert abs(t.cost - d.cost) <= 1e-7 * abs(t.cost)
        assert not (np.array_equal(t.H_np(), d.H_np()) and np.array_equal(t.b_np(), d.b_np()))
    # the mode is reset afterwards: a plain evaluation gives the plain bits again
    again = o.eval_normal(p, xs, nthreads=1)
    for a, b in zip(again, plain):
        assert np.array_equal(a.H_np(), b.H_np()) and np.array_equal(a.b_np(), b.b_np()) and a.cost == b.cost


def _normal(H, b, cost, chi2, counts=(10, 20, 30, 40)):
    return SimpleNamespace(H_np=lambda: np.array(H), b_np=lambda: np.array(b), cost=cost, chi2=chi2, counts=lambda: counts)


def _synthetic(rng):
    """a truth t, a double oracle o that is 1e-9 (relative) off it on every entry, and the direction d of that error"""
    J = rng.normal(size=(40, 7))
    H = J.T @ J + 7 * np.eye(7)
    b = rng.normal(size=7) * 10
    dH, db = rng.choice([-1.0, 1.0], size=(7, 7)), rng.choice([-1.0, 1.0], size=7)
    t = _normal(H, b, 123.0, 246.0)
    o = _normal(H * (1 + 1e-9 * dH), b * (1 + 1e-9 * db), 123.0 * (1 + 1e-9), 246.0 * (1 - 1e-9))
    return t, o, (H, b, dH, db)


def test_the_gate_has_teeth():
    t, o, (H, b, dH, db) = _synthetic(np.random.default_rng(0))
    # the device as close as the oracle, and within SLACK of its error: passes
    for f in (0.0, 0.5, 1.0, 1.4):
        g = _normal(H * (1 - f * 1e-9 * dH), b * (1 + f * 1e-9 * db), 123.0 * (1 - f * 1e-9), 246.0 * (1 + f * 1e-9))
        ok, rep = parity_gate.check_normal_vs_truth(g, o, t)
        assert ok, (f, rep)
        parity_gate.normal_vs_truth(g, o, t)
    # three times the oracle's error on H, on b, on the cost, on chi^2 alone: fails, and says where
    bad = {"H": _normal(H * (1 + 3e-9 * dH), b, 123.0, 246.0), "b": _normal(H, b * (1 - 3e-9 * db), 123.0, 246.0),
           "cost": _normal(H, b, 123.0 * (1 + 3e-9), 246.0), "chi2": _normal(H, b, 123.0, 246.0 * (1 - 3e-9))}
    for k, g in bad.items():
        ok, rep = parity_gate.check_normal_vs_truth(g, o, t)
        assert not ok and rep["failed"] == [k], (k, rep)
        with pytest.raises(AssertionError):
            parity_gate.normal_vs_truth(g, o, t)
    assert parity_gate.check_normal_vs_truth(bad["H"], o, t)[1]["H"]["device"][0] == pytest.approx(3e-9, rel=1e-3)
    # one small entry (below FLOOR of the largest) moved by three times the oracle's error there: fails too
    Hs = H.copy(); Hs[0, 1] = Hs[1, 0] = 1e-9 * np.abs(H).max()
    Ho, Hg = Hs.copy(), Hs.copy()
    Ho[0, 1] += 1e-15 * np.abs(H).max()
    Hg[0, 1] += 3e-15 * np.abs(H).max()
    ok, rep = parity_gate.check_normal_vs_truth(_normal(Hg, b, 123.0, 246.0), _normal(Ho, b, 123.0, 246.0), _normal(Hs, b, 123.0, 246.0))
    assert not ok and rep["failed"] == ["H"], rep
    # an oracle that is exact: the device is held to REL (1e-10) of the truth
    ok, _ = parity_gate.check_normal_vs_truth(_normal(H * (1 + 0.9e-10), b, 123.0, 246.0), t, t)
    assert ok
    ok, rep = parity_gate.check_normal_vs_truth(_normal(H * (1 + 1.2e-10), b, 123.0, 246.0), t, t)
    assert not ok and rep["failed"] == ["H"]
    # a counter that differs: fails whatever the sums
    g = _normal(H, b, 123.0, 246.0, counts=(10, 20, 30, 41))
    ok, rep = parity_gate.check_normal_vs_truth(g, o, t)
    assert not ok and "counts" in rep["failed"]
    with pytest.raises(AssertionError):
        parity_gate.normal_vs_truth(g, o, t)


def test_the_cap_on_explained_candidates():
    parity_gate.explained_within([], [], 0, 0)
    parity_gate.explained_within([3, 17], [1, 2], 2, 3)
    with pytest.raises(AssertionError):
        parity_gate.explained_within([3, 17, 40], [1, 1, 1], 2, 10)      # one candidate too many
    with pytest.raises(AssertionError):
        parity_gate.explained_within([3, 17], [2, 2], 2, 3)              # one flagged block too many
    with pytest.raises(AssertionError):
        parity_gate.explained_within([3, 17], [2], 2, 3)                 # a candidate without its block count
