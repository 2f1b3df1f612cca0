"""The constant-velocity motion model of the live tracker: what needs no device -- the rule that measures the expected
motion and the prediction on an exact constant-velocity trajectory, the float64 restatement (tests/live_motion_restated.py) against a
complex-step derivative and a dense Schur complement, the parameter checks of include/aar.h, and the benefit on a coasting stream.  CPU only.

Measured while writing this test (restatement, tests/live_motion_cases.moving_stream: 2 degrees and 10 mm per unit of time, 0.3 px, lag 3, sigmas
0.05 / 0.02, frames 12 .. 15 emptied): newest-pose error with the model over the random walk's at the four emptied frames 0.024, 0.015, 0.012,
0.011 in rotation and 0.029, 0.019, 0.015, 0.013 in translation -- below the 1/8 the issue asks to explain, far below the 1/4 asserted."""
import copy
import ctypes as C

import numpy as np
import pytest

import aar
import live_marginal_cases as mc
import live_marginal_restated as lm
import live_motion_cases as mcv
import live_motion_restated as mr
import smooth_restated as sr
import track_restated as tr


# ---- 1. the rule on an exact constant-velocity trajectory ----
def test_exact_constant_velocity_trajectory():
    t = mc.times(16)
    assert len(set(np.round(np.diff(t), 12))) > 1                          # uneven: s != 1
    vel = np.array([0.031, -0.022, 0.017, 0.012, -0.007, 0.004])
    z = mcv.constant_velocity_poses(np.array([0.4, -0.7, 0.3, 0.1, -0.2, 1.5]), vel, t)
    scales = set()
    for n in range(2, len(t)):
        rel, pred, predicted = mr.measure(z[n - 2], z[n - 1], t[n - 2], t[n - 1], t[n])
        scales.add(round((t[n] - t[n - 1]) / (t[n - 1] - t[n - 2]), 9))
        assert predicted
        assert np.abs(sr.between(z[n - 1], z[n], rel)).max() < 1e-12, n
        assert np.abs(pred - z[n]).max() < 1e-12, n
        np.testing.assert_allclose(rel, vel * (t[n] - t[n - 1]), rtol=0, atol=1e-12)
        np.testing.assert_allclose(mr.velocity(z[n - 1], z[n], t[n - 1], t[n]), vel, rtol=0, atol=1e-12)
        assert np.abs(mr.predict(z[n - 1], vel, t[n - 1], t[n]) - z[n]).max() < 1e-12
    assert {1.0, 5.0, 0.2} <= scales
    # without the scaling, or with the world / body conventions exchanged, the error does not vanish
    rel, _, _ = mr.measure(z[3], z[4], t[3], t[4], t[5])
    assert np.abs(sr.between(z[4], z[5], rel * (t[4] - t[3]) / (t[5] - t[4]))).max() > 1e-3
    Ra, Rb = tr.rodrigues(z[3][:3]), tr.rodrigues(z[4][:3])
    world = np.r_[sr.so3_log(Rb @ Ra.T), rel[3:]]
    assert np.abs(sr.between(z[4], z[5], world)).max() > 1e-4


def test_rule_is_zero_before_two_frames_and_across_a_gap():
    za, zb = np.array([0.1, 0.2, 0.3, 0.0, 0.1, 1.0]), np.array([0.12, 0.2, 0.31, 0.01, 0.1, 1.02])
    rel, pred, predicted = mr.measure(None, zb, None, 1.0, 2.0)
    assert not predicted and not rel.any() and np.array_equal(pred, zb)
    for ta, tb, time, want in [(0.0, 1.0, 2.0, True), (0.0, 1.0, 3.5, False), (0.0, 2.5, 3.0, False), (0.0, 2.0, 4.0, True)]:
        rel, pred, predicted = mr.measure(za, zb, ta, tb, time, max_dt=2.0)
        assert predicted == want
        assert rel.any() == want and (want or np.array_equal(pred, zb))
    assert np.array_equal(mr.predict(zb, np.ones(6), 1.0, 3.5, max_dt=2.0), zb)


# ---- 2. the restatement against itself ----
def _window(lag=3, anchor="fixed", pushes=8):
    """a LiveCV window problem in mid-stream, its point and the restated push"""
    rs = mcv.restated("counts", lag, anchor)
    r = rs[pushes]
    return r["problem"], r["start"], r


@pytest.mark.parametrize("anchor", ["fixed", "marginal"])
def test_gradient_against_a_complex_step_of_the_cost(anchor):
    wp, z, r = _window(3, anchor)
    assert wp.rel[1:].any() and wp.F == 4 and (wp.prior is not None) == (anchor == "marginal")
    z = z + 1e-3 * np.random.default_rng(3).normal(size=z.shape)           # away from the start, where nothing is special
    _, _, rhs = wp.system(z)
    h = 1e-30
    g = np.zeros(z.size)
    for k in range(z.size):
        zc = z.astype(complex).reshape(-1)
        zc[k] += 1j * h
        g[k] = wp.cost_complex(zc.reshape(z.shape)).imag / h
    np.testing.assert_allclose(wp.cost_complex(z.astype(complex)).real, wp.cost(z), rtol=1e-13)
    scale = np.abs(g).max()
    assert np.abs(-0.5 * g - rhs).max() <= 1e-9 * scale                    # b = -J^T r = -grad / 2
    # the expected motion matters: the same window without it has another gradient
    wp0 = copy.copy(wp)
    wp0.rel = np.zeros_like(wp.rel)
    assert np.abs(wp0.system(z)[2] - rhs).max() > 1e-6 * scale             # (a thousand times the bar above)


@pytest.mark.parametrize("lag", [1, 3])
def test_marginal_against_the_schur_complement_of_the_dense_hessian(lag):
    wp, _, r = _window(lag, "marginal", 9)
    zf = r["window"]
    assert wp.rel[1].any()
    Lp, bp, B = mr.marginal_terms(wp, zf)
    # the energy that involves frame 0: everything of its block row, and of frame 1 only the J_b half of pair (0, 1)
    diag, off, rhs = wp.system(zf)
    H = np.zeros((12, 12))
    H[:6, :6], H[:6, 6:], H[6:, :6], H[6:, 6:] = diag[0], off[0], off[0].T, B
    J, e = sr.between_jacobian(zf[0], zf[1], wp.rel[1])
    g = np.r_[rhs[:6], -J[:, 6:].T @ (wp.lam[1] * e)]
    S = H[6:, 6:] - H[6:, :6] @ np.linalg.solve(H[:6, :6], H[:6, 6:])
    s = g[6:] - H[6:, :6] @ np.linalg.solve(H[:6, :6], g[:6])
    assert np.abs(S - Lp).max() <= 1e-9 * np.abs(Lp).max() and np.abs(s - bp).max() <= 1e-9 * max(np.abs(bp).max(), 1.0)
    got = mr.marginalise(wp, zf)
    assert got is not None
    np.testing.assert_allclose(got[1], zf[1] + np.linalg.solve(S, s), rtol=0, atol=1e-9)
    # ... and it is not the marginal of the random walk
    L0, b0, _ = lm.marginal_terms(wp, zf)
    assert np.abs(b0 - bp).max() > 1e-6 * np.abs(bp).max()


def test_driver_without_the_model_is_the_random_walk_restatement():
    c = mc.case("counts", 3)
    ref = mc.restated("counts", 3, "marginal")
    live = mr.LiveCV(c.td, lag=3, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, anchor="marginal", model=False)
    for f in range(c.n):
        r = live.push(f, c.times[f], pose_init=c.td.z0[f] if c.has_init[f] else None)
        assert r["iterations"] == ref[f]["iterations"] and r["err"] == ref[f]["err"] and np.array_equal(r["pose"], ref[f]["pose"]), f


# ---- 3. validation and lifecycle ----
def test_defaults_and_struct_sizes():
    p = aar.tracker_motion_params()
    assert (p.model, p.max_dt) == (aar.TRACKER_MOTIONS["cv"], 0.0) and p.model == 1
    assert p.struct_size == C.sizeof(aar.CTrackerMotionParams) == 16
    assert C.sizeof(aar.CTrackerMotionInfo) == 120 and aar.CTrackerMotionInfo.rel.offset == 16 and aar.CTrackerMotionInfo.newest_time.offset == 112
    aar.tracker_motion_params_validate()
    aar.tracker_motion_params_validate(max_dt=2.5)
    aar.tracker_motion_params_validate(model="rw")
    aar.tracker_motion_params_validate(model="rw", tracker=dict(smooth=False))      # the random walk needs no prior to be the random walk
    aar.tracker_motion_params_validate(struct_size=8)                       # just reaches model: max_dt at its default
    aar.tracker_motion_params_validate(struct_size=64)                      # a longer (newer) struct: the known fields are read
    aar.tracker_motion_params_validate(tracker=dict(lag=15, smooth=True, sigma_rot=1.0, sigma_trans=1.0, anchor="marginal"))


@pytest.mark.parametrize("kw,field", [
    (dict(struct_size=7), "struct_size"), (dict(struct_size=4), "struct_size"),
    (dict(model=2), "model"), (dict(model=-1), "model"),
    (dict(max_dt=-1.0), "max_dt"), (dict(max_dt=float("nan")), "max_dt"), (dict(max_dt=float("inf")), "max_dt"),
    (dict(tracker=dict(smooth=False)), "smooth")])
def test_validate_refuses_and_names_the_field(kw, field):
    with pytest.raises(aar.AarError) as e:
        aar.tracker_motion_params_validate(**kw)
    assert e.value.code == aar.AAR_ERR_INVALID
    assert "aar_tracker_motion_params" in str(e.value) and field in str(e.value)


def test_null_arguments_are_refused_without_a_device():
    L = aar.lib()
    p, tp = aar.tracker_motion_params(), aar.tracker_params(smooth=True, sigma_rot=1.0, sigma_trans=1.0)
    assert L.aar_tracker_motion_params_validate(None, C.byref(p)) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_motion_params_validate(C.byref(tp), None) == aar.AAR_ERR_INVALID
    assert L.aar_tracker_enable_motion(None, None) == aar.AAR_ERR_INVALID
    m = aar.CTrackerMotionInfo()
    m.struct_size = C.sizeof(m)
    assert L.aar_tracker_last_motion(None, C.byref(m)) == aar.AAR_ERR_INVALID
    pose = np.zeros(6)
    assert L.aar_tracker_predict(None, 1.0, pose.ctypes.data_as(C.POINTER(C.c_double))) == aar.AAR_ERR_INVALID
    L.aar_tracker_default_motion_params(None)                               # tolerated, as its neighbours


# ---- 4. the benefit, on the restatement ----
def test_coasting_error_is_a_quarter_of_the_random_walks_at_most():
    c = mcv.moving_stream()
    cnt = np.bincount(c.ds.obs_frame, minlength=c.n)
    assert [f for f in range(c.n) if cnt[f] == 0] == list(c.empty) and len(c.empty) == 4
    step = mcv.pose_errors(c.truth[1], c.truth[0])
    np.testing.assert_allclose(step, [np.deg2rad(2.0), 0.010], rtol=1e-9)   # 2 degrees and 10 mm per unit of time
    cv, rw = mcv.coast_restated(True), mcv.coast_restated(False)
    for f in c.empty:
        (ar, at), (br, bt) = mcv.pose_errors(cv[f]["pose"], c.truth[f]), mcv.pose_errors(rw[f]["pose"], c.truth[f])
        print("frame %d: rotation %.3e / %.3e = %.4f, translation %.3e / %.3e = %.4f" % (f, ar, br, ar / br, at, bt, at / bt))
        assert ar <= 0.25 * br and at <= 0.25 * bt, f
        assert cv[f]["predicted"] == 1 and cv[f]["iterations"] <= 1
    # where the object is seen the two agree closely at these sigmas (printed, not asserted: the issue sets no bar there)
    seen = [f for f in range(2, c.n) if f not in c.empty]
    e_cv = np.mean([mcv.pose_errors(cv[f]["pose"], c.truth[f]) for f in seen], axis=0)
    e_rw = np.mean([mcv.pose_errors(rw[f]["pose"], c.truth[f]) for f in seen], axis=0)
    print("seen frames: mean error with the model %s, random walk %s" % (e_cv, e_rw))
