"""The float64 restatement of the live tracker (tests/live_restated.py) against the restatements it is built on, and the host side of the
aar_tracker_* entry points (parameter validation, exported symbols).  CPU only."""
import ctypes as C

import numpy as np
import pytest

import aar
import live_restated as lr
import smooth_cases as sc
import smooth_restated as sr
import track_restated as tr

SROT, STRANS = 0.05, 0.02


@pytest.fixture(scope="module")
def small():
    ds = aar.synth(2, num_frames=6)
    x0 = sc.track_start(ds)
    return ds, x0, tr.TrackData(ds, x0)


TIMES = np.array([0.0, 1.0, 2.5, 3.5, 8.0, 9.0])


@pytest.mark.parametrize("delta", [None, 0.5])
def test_anchored_system_is_the_joint_system_with_the_anchor_struck_out(small, delta):
    ds, x0, td = small
    z = td.z0.copy()
    joint = sr.SmoothProblem(td, SROT, STRANS, delta=delta, frame_time=TIMES)
    diag, off, rhs = joint.system(z)
    Ef, Pe = joint.costs(z)
    wp = lr.WindowProblem(td, range(1, 6), TIMES[1:], SROT, STRANS, delta=delta, anchor=(z[0], TIMES[0]))
    d2, o2, r2 = wp.system(z[1:])
    big = max(np.abs(diag).max(), np.abs(off).max())
    assert np.abs(d2 - diag[1:]).max() <= 1e-13 * big
    assert np.abs(o2 - off[1:]).max() <= 1e-13 * big
    assert np.abs(r2 - rhs[6:]).max() <= 1e-13 * np.abs(rhs).max()
    E2, P2 = wp.costs(z[1:])
    np.testing.assert_allclose(E2, Ef[1:], rtol=1e-13)
    np.testing.assert_allclose(P2, Pe, rtol=1e-13)                 # P2[0] is the anchor pair = the joint problem's pair (0, 1)
    assert wp.rows == joint.rows - 8.0 * (td.start[1] - td.start[0])
    # without an anchor: the joint system of the window's frames alone
    sub = sc.copy_of(ds, num_frames=5, frame_ids=ds.frame_ids[1:], obs_frame=ds.obs_frame[ds.obs_frame > 0] - 1, obs_cam=ds.obs_cam[ds.obs_frame > 0],
                     obs_marker=ds.obs_marker[ds.obs_frame > 0], obs_uv=ds.obs_uv[ds.obs_frame > 0],
                     x_full=np.r_[x0[:sc.ns(ds)], x0[sc.ns(ds) + 6:]])
    js = sr.SmoothProblem(tr.TrackData(sub, sub.x_full), SROT, STRANS, delta=delta, frame_time=TIMES[1:])
    d3, o3, r3 = js.system(z[1:])
    w0 = lr.WindowProblem(td, range(1, 6), TIMES[1:], SROT, STRANS, delta=delta)
    d4, o4, r4 = w0.system(z[1:])
    assert np.abs(d4 - d3).max() <= 1e-13 * big and np.abs(o4 - o3).max() <= 1e-13 * big and np.abs(r4 - r3).max() <= 1e-13 * np.abs(r3).max()
    assert w0.rows == js.rows and w0.costs(z[1:])[1][0] == 0.0


def test_anchor_half_against_a_complex_step_on_between(small):
    ds, x0, td = small
    z = td.z0.copy()
    za, t_a = z[0], TIMES[0]
    with_a = lr.WindowProblem(td, [1, 2], TIMES[1:3], SROT, STRANS, anchor=(za, t_a))
    without = lr.WindowProblem(td, [1, 2], TIMES[1:3], SROT, STRANS)
    dA, _, rA = with_a.system(z[1:3])
    d0, _, r0 = without.system(z[1:3])
    h = 1e-30
    zb = z[1][None, :] + 1j * h * np.eye(6)
    Jb = (sr.between(np.broadcast_to(za, (6, 6)), zb).imag / h).T        # [6, 6] d e / d z_first, the anchor constant
    e = sr.between(za, z[1])
    L = np.r_[[1.0 / (SROT * SROT * (TIMES[1] - t_a))] * 3, [1.0 / (STRANS * STRANS * (TIMES[1] - t_a))] * 3]
    H = Jb.T @ (L[:, None] * Jb)
    g = -Jb.T @ (L * e)
    assert np.abs((dA[0] - d0[0]) - H).max() <= 1e-11 * np.abs(H).max()
    assert np.abs((rA[:6] - r0[:6]) - g).max() <= 1e-11 * np.abs(g).max()
    assert np.array_equal(dA[1], d0[1]) and np.array_equal(rA[6:], r0[6:])      # the anchor touches the first frame only
    np.testing.assert_allclose(with_a.costs(z[1:3])[1][0], float(np.sum(L * e * e)), rtol=1e-13)


@pytest.mark.parametrize("delta", [-1.0, 0.5])
def test_smooth_0_push_is_track_frame(small, delta):
    ds, x0, td = small
    live = lr.Live(td, lag=0, smooth=False, delta=delta)
    for f in range(ds.num_frames):
        ref = tr.track_frame(td.frame(f), td.z0[f], delta=delta)
        r = live.push(f, float(f), pose_init=td.z0[f])
        assert (r["iterations"], r["exit"], r["rejected"]) == (ref["iterations"], ref["exit"], ref["rejected"])
        assert r["window_frames"] == 1 and r["prior"] == 0.0
        np.testing.assert_allclose(r["err"], ref["err"], rtol=1e-12)
        assert np.abs(r["pose"] - ref["z"]).max() < 1e-12
        assert np.array_equal(r["lagged_pose"], r["pose"])


def test_driver_carries_window_anchor_and_starts(small):
    ds, x0, td = small
    live = lr.Live(td, lag=2, smooth=True, sigma_rot=SROT, sigma_trans=STRANS)
    lagged = {}
    for f in range(6):
        before = [w[2].copy() for w in live.win]
        r = live.push(f, TIMES[f], pose_init=td.z0[f] if f % 2 == 0 else None)
        wp = r["problem"]
        assert r["window_frames"] == min(f + 1, 3) and wp.frames == list(range(max(0, f - 2), f + 1))
        assert (wp.anchor is not None) == (f >= 3)
        if f >= 3:
            assert np.array_equal(wp.anchor, lagged[f - 3])             # the anchor is the pose last reported as lagged
        assert wp.rows == 8.0 * (td.start[f + 1] - td.start[max(0, f - 2)]) + 6.0 * (min(f, 2) + (f >= 3))
        if r["lagged_pose"] is not None:
            lagged[f - 2] = r["lagged_pose"]
        assert r["err"] <= wp.cost(np.stack((before[-2:] if f >= 3 else before) + [td.z0[f] if f % 2 == 0 else before[-1]])) + 1e-12
    live.reset()
    assert live.n == 0 and live.anchor is None


# ---- the host side of the C ABI ----
def test_params_validate_names_the_field(small):
    ds = small[0]
    aar.tracker_params_validate(ds, lag=0, smooth=False)
    aar.tracker_params_validate(ds, lag=15, smooth=True, sigma_rot=SROT, sigma_trans=STRANS, with_huber=True, huber_delta=0.5)
    good = dict(lag=3, smooth=True, sigma_rot=SROT, sigma_trans=STRANS)
    cases = [(dict(good, lag=16), "lag"), (dict(good, lag=-1), "lag"), (dict(lag=1, smooth=False), "lag"),
             (dict(good, sigma_rot=0.0), "sigma_rot"), (dict(good, sigma_rot=np.inf), "sigma_rot"), (dict(good, sigma_rot=np.nan), "sigma_rot"),
             (dict(good, sigma_trans=-1.0), "sigma_trans"), (dict(good, sigma_trans=np.inf), "sigma_trans"),
             (dict(good, max_obs_per_frame=0), "max_obs_per_frame"), (dict(good, with_huber=True, huber_delta=0.0), "huber_delta"),
             (dict(good, struct_size=4), "struct_size")]
    for kw, word in cases:
        with pytest.raises(aar.AarError) as e:
            aar.tracker_params_validate(ds, **kw)
        assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), (kw, str(e.value))
    aar.tracker_params_validate(ds, lag=0, smooth=False, sigma_rot=-1.0)          # the sigmas only count with smooth
    # malformed solutions
    for over, word in [(dict(root_cam=ds.num_cams), "root_cam"), (dict(root_marker=-1), "root_marker"), (dict(marker_size=0.0), "marker_size"),
                       (dict(num_cams=0), "cameras")]:
        bad = sc.copy_of(ds, **over)
        with pytest.raises(aar.AarError) as e:
            aar.tracker_params_validate(bad, **good)
        assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), (over, str(e.value))
    x = np.array(ds.x_full)
    x[7] = np.nan
    with pytest.raises(aar.AarError) as e:
        aar.tracker_params_validate(sc.copy_of(ds, x_full=x), **good)
    assert e.value.code == aar.AAR_ERR_INVALID and "x_full[7]" in str(e.value)


def test_new_symbols_are_exported():
    names = ["aar_tracker_default_params", "aar_tracker_params_validate", "aar_tracker_create", "aar_tracker_push", "aar_tracker_window",
             "aar_tracker_reset", "aar_tracker_destroy"]
    lib = C.CDLL(aar.LIB_PATH)
    for n in names:
        assert hasattr(lib, n) and n in aar.SYMBOLS, n
    p = aar.tracker_params()
    assert p.struct_size == C.sizeof(aar.CTrackerParams) and (p.lag, p.smooth, p.with_huber, p.max_obs_per_frame) == (0, 0, 0, 256)
    assert aar.TRACKER_MAX_LAG == 15


def test_create_needs_a_device_and_valid_params(small):
    ds = small[0]
    with pytest.raises(aar.AarError) as e:
        aar.Tracker(ds, lag=2, smooth=False)                      # validated before the device is touched
    assert e.value.code == aar.AAR_ERR_INVALID
    if aar.device_count() == 0:
        with pytest.raises(aar.AarError) as e:
            aar.Tracker(ds)
        assert e.value.code == aar.AAR_ERR_NO_DEVICE
