"""Inputs of the constant-velocity query tests (tests/test_smooth_cv_query_host.py, tests/test_gpu_track_smooth_cv_query.py) -- TEST
INFRASTRUCTURE ONLY."""
import numpy as np

import aar
import projection_reference as pr
import smooth_cases as sc
import smooth_cv_query_restated as scq
import smooth_query_cases as sqc

frames_of = sqc.frames_of


def inserted(ds, x_full, frame_time, t, zm=None):
    """The AUGMENTED problem of a query at t (not a frame time) under the constant-velocity model, after smooth_query_cases.inserted: a frame
    without detections inserted at t at the START POSE of the definition (the geodesic inside a gap, the constant-velocity extrapolation
    outside; zm: that pose as somebody else computed it, the device for instance).  Returns (data set, x_full, frame_time, its index)."""
    F = ds.num_frames
    times = scq.times_of(F, frame_time)
    a, kind = scq.locate(times, t)
    assert kind != "on"
    pos = a + 1
    z = frames_of(ds, x_full)
    zm = scq.start_pose(z, times, t) if zm is None else np.asarray(zm, dtype=np.float64)
    n0 = sc.ns(ds)
    x = np.asarray(x_full)
    z2 = np.concatenate([z[:pos], zm[None, :], z[pos:]])
    frame = np.asarray(ds.obs_frame)
    out = sc.copy_of(ds, num_frames=F + 1, frame_ids=np.arange(F + 1, dtype=np.int32),
                     obs_frame=(frame + (frame >= pos)).astype(frame.dtype), x_full=np.concatenate([x[:n0], z2.reshape(-1), x[n0 + 6 * F:]]),
                     x_truth=None)
    return out, np.array(out.x_full), np.concatenate([times[:pos], [t], times[pos:]]), pos


def embedded(rhs, pos):
    """the original right-hand side [6F] with zero at the inserted frame: [6 (F + 1)]"""
    g = np.asarray(rhs).reshape(-1, 6)
    return np.concatenate([g[:pos], np.zeros((1, 6)), g[pos:]]).reshape(-1)


def yardstick(H2, g2, g, pos):
    """(cov [6, 6], delta_m [6], |delta|_inf of the full step, kappa_2(H')) from the dense augmented system H', its right-hand side g' and
    the original g"""
    Hi = np.linalg.inv(H2)
    step = np.linalg.solve(H2, g2 - embedded(g, pos))
    ev = np.linalg.eigvalsh(H2)
    assert ev[0] > 0
    return Hi[6 * pos:6 * pos + 6, 6 * pos:6 * pos + 6], step[6 * pos:6 * pos + 6], float(np.abs(step).max()), float(ev[-1] / ev[0])


def translating_sequence(n_frames=10, config=2):
    """A noiseless object that only translates, on a curved path and uneven frame times (after smooth_cv_cases.constant_velocity_sequence):
    R_f = R_0, t_f = t_0 + tau_f v + a sin(tau_f / 3).  Returns (ds with the first, the last and an inner frame emptied, x0 = every frame at the
    first frame's pose, truth poses [F, 6], frame_time, emptied frames)."""
    base = aar.synth(config)
    cnt = np.bincount(base.obs_frame, minlength=base.num_frames)
    f0 = int(cnt.argmax())
    sel = np.nonzero(base.obs_frame == f0)[0]
    n = len(sel)
    n0 = sc.ns(base)
    z0 = np.array(base.x_truth[n0 + 6 * f0: n0 + 6 * f0 + 6])
    ft = np.cumsum(np.r_[0.0, 1.0 + 0.5 * (np.arange(n_frames - 1) % 3)])
    v, a = np.array([0.004, -0.002, 0.003]), np.array([0.01, 0.02, -0.015])
    zt = np.stack([np.r_[z0[:3], z0[3:] + t * v + np.sin(t / 3.0) * a] for t in ft])
    truth = np.concatenate([base.x_truth[:n0], zt.reshape(-1)])
    ds = sc.copy_of(base, num_frames=n_frames, frame_ids=np.arange(n_frames, dtype=np.int32),
                    obs_frame=np.repeat(np.arange(n_frames, dtype=np.int32), n), obs_cam=np.tile(base.obs_cam[sel], n_frames),
                    obs_marker=np.tile(base.obs_marker[sel], n_frames), obs_uv=np.zeros((n * n_frames, 8), dtype=np.float32),
                    x_truth=truth, x_full=np.concatenate([base.x_truth[:n0], np.tile(zt[0], n_frames)]))
    ds.obs_uv = pr.Reference(ds).projection(truth).astype(np.float32)
    empty = [0, n_frames // 2, n_frames - 1]
    return sc.without_frames(ds, empty), np.array(ds.x_full), zt, ft, empty
