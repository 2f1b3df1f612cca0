"""Inputs of the motion-model tests of the live tracker (tests/test_live_motion_host.py, tests/test_gpu_live_motion.py) -- TEST INFRASTRUCTURE
ONLY.  The stream cases are those of tests/live_marginal_cases.py (uneven push times, a pose_init on two pushes of three); the restated runs
are computed once per case and shared.  moving_stream is the coasting case: an object at constant velocity with four emptied frames."""
import functools
from types import SimpleNamespace

import numpy as np

import aar
import live_marginal_cases as mc
import live_motion_restated as mr
import projection_reference as pr
import smooth_cases as sc
import smooth_restated as sr
import track_restated as tr

MAX_DT = 2.0          # between the short (1) and the long (5) gaps of live_marginal_cases.times


@functools.lru_cache(maxsize=None)
def restated(kind, lag, anchor, max_dt=0.0):
    """every push of live_marginal_cases.case(kind, lag) by live_motion_restated.LiveCV (each dict also carries window and anchor after the push)"""
    c = mc.case(kind, lag)
    live = mr.LiveCV(c.td, lag=c.lag, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, delta=-1.0 if c.delta is None else c.delta, anchor=anchor,
                     max_dt=max_dt, **c.lm)
    out = []
    for f in range(c.n):
        r = live.push(f, c.times[f], pose_init=c.td.z0[f] if c.has_init[f] else None)
        r["window"], r["anchor"] = live.window()
        out.append(r)
    return out


def constant_velocity_poses(z0, vel, t):
    """R_n = R_0 exp(omega t_n), t_n = t_0 + v t_n as [n, 6] (rvec, t)"""
    R0 = tr.rodrigues(np.asarray(z0[:3], dtype=np.float64))
    return np.stack([np.concatenate([sr.so3_log(R0 @ tr.rodrigues(vel[:3] * tn)), z0[3:] + vel[3:] * tn]) for tn in t])


# the coasting stream: 2 degrees and 10 mm per unit of time, 0.3 px noise, lag 3, frames 12 .. 15 without detections (behind the hole 10 -> 11 of
# the times, so that rel_12 is scaled by s = 1 / 5)
COAST_N, COAST_LAG, COAST_EMPTY, COAST_NOISE = 20, 3, (12, 13, 14, 15), 0.3
COAST_VEL = np.r_[np.deg2rad(2.0) * np.array([0.6, -0.64, 0.48]), 0.010 * np.array([0.8, 0.0, -0.6])]


@functools.lru_cache(maxsize=None)
def moving_stream(seed=5):
    """live_marginal_cases.moving_object's construction on the four-camera scene with COAST_VEL: the best-observed frame of the scene's truth
    carried along the constant-velocity trajectory, its detections replicated with fresh corner noise, the emptied frames left without any."""
    n = COAST_N
    base = aar.synth(3, num_cams=4, num_markers=8, num_frames=8, noise_px=0.0, min_view_cos=0.3)
    cnt = np.bincount(base.obs_frame, minlength=base.num_frames)
    f0 = int(cnt.argmax())
    sel = np.nonzero(base.obs_frame == f0)[0]
    k = len(sel)
    n0 = sc.ns(base)
    zt = np.array(base.x_truth[n0 + 6 * f0: n0 + 6 * f0 + 6])
    t = mc.times(n)
    truth_z = constant_velocity_poses(zt, COAST_VEL, t - t[n // 2])            # the observed pose in the middle of the stream
    truth = np.concatenate([base.x_truth[:n0], truth_z.reshape(-1)])
    ds = sc.copy_of(base, num_frames=n, frame_ids=np.arange(n, dtype=np.int32), obs_frame=np.repeat(np.arange(n, dtype=np.int32), k),
                    obs_cam=np.tile(base.obs_cam[sel], n), obs_marker=np.tile(base.obs_marker[sel], n), obs_uv=np.zeros((k * n, 8), dtype=np.float32),
                    x_truth=truth, x_full=truth.copy())
    uv = pr.Reference(ds).projection(truth)
    assert np.all(np.isfinite(uv)) and np.abs(uv).max() < 1e4
    rng = np.random.default_rng(seed)
    ds.obs_uv = (uv + rng.normal(0.0, COAST_NOISE, size=uv.shape)).astype(np.float32)
    ds = mc.keep_first(ds, [0 if f in COAST_EMPTY else None for f in range(n)])
    x0 = np.array(ds.x_truth)          # cameras and markers at the truth: the tracker's solution
    td = tr.TrackData(ds, x0)
    kw = dict(lag=COAST_LAG, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, max_obs_per_frame=k)
    return SimpleNamespace(name="coast", ds=ds, td=td, n=n, lag=COAST_LAG, times=t, truth=truth_z, kw=kw, sol=sc.copy_of(ds, x_full=x0),
                           empty=COAST_EMPTY, delta=None, lm={}, has_init=[f == 0 for f in range(n)])


@functools.lru_cache(maxsize=None)
def coast_restated(model):
    """the coasting stream by LiveCV with (True) and without (False) the model; the first push starts from the truth, no other pose_init"""
    c = moving_stream()
    live = mr.LiveCV(c.td, lag=c.lag, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, model=model)
    out = []
    for f in range(c.n):
        r = live.push(f, c.times[f], pose_init=c.truth[0] if f == 0 else None)
        r["window"], r["anchor"] = live.window()
        out.append(r)
    return out


def pose_errors(z, zt):
    """(rotation angle [rad], translation distance) between poses z and zt"""
    e = sr.between(zt, z)
    return float(np.linalg.norm(e[:3])), float(np.linalg.norm(e[3:]))
