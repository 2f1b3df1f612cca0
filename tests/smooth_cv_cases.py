"""Inputs of the constant-velocity smoothing tests (tests/test_smooth_cv_host.py, tests/test_gpu_track_smooth_cv.py) -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

import aar
import projection_reference as pr
import smooth_cases as sc
import smooth_restated as sr
import track_restated as tr

SROT, STRANS = 0.05, 0.02      # the random-walk tests' sigmas: here the deviation from constant velocity per sqrt(frame)
SROT0, STRANS0 = 1.0, 1.0      # pair 0: a loose prior on the first velocity
# the average-step stop off (a frame without detections moves on the prior's small cost alone) and 14 iterations: the claim case has then
# converged to 1e-7 and every decision of the restated run is still decided (margin 3e-6; from iteration 17 on they are rounding's)
TIGHT = dict(min_avg=0.0, max_iters=14)


def gaps(F):
    """frame times with a hole of five every seventh frame (as tests/test_gpu_track_smooth.py)"""
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(F - 1) % 7 == 3) * 4.0])


def claim_case():
    """config 2 (4 cameras, 12 markers, 100 frames) with the first, the last and ten inner frames emptied: (ds, x0, emptied frames)"""
    ds0 = aar.synth(2)
    x0 = sc.track_start(ds0)
    empty = sc.emptied(ds0.num_frames)
    return sc.without_frames(ds0, empty), x0, empty


def end_errors(z, ds):
    """|z_f - truth_f| (all six entries) of the first and the last frame"""
    n0 = sc.ns(ds)
    zt = np.asarray(ds.x_truth)[n0: n0 + 6 * ds.num_frames].reshape(-1, 6)
    z = np.asarray(z).reshape(-1, 6)
    return float(np.linalg.norm(z[0] - zt[0])), float(np.linalg.norm(z[-1] - zt[-1]))


def constant_velocity_sequence(n_frames=12, config=2):
    """A noiseless object in exactly constant motion on uneven frame times: R_f = R_0 Exp(tau_f w), t_f = t_0 + tau_f v, the best-observed
    frame's observation list of the config replicated and projected through tests/projection_reference.py.  Returns (ds with the first, the
    last and an inner frame emptied, x0 = every frame at the first frame's pose, truth poses [F, 6], frame_time, emptied frames, |w|)."""
    base = aar.synth(config)
    cnt = np.bincount(base.obs_frame, minlength=base.num_frames)
    f0 = int(cnt.argmax())
    sel = np.nonzero(base.obs_frame == f0)[0]
    n = len(sel)
    n0 = sc.ns(base)
    z0 = np.array(base.x_truth[n0 + 6 * f0: n0 + 6 * f0 + 6])
    ft = np.cumsum(np.r_[0.0, 1.0 + 0.5 * (np.arange(n_frames - 1) % 3)])          # steps 1, 1.5, 2, 1, ...
    w, v = np.array([0.02, -0.025, 0.03]), np.array([0.004, -0.002, 0.003])
    R0 = tr.rodrigues(z0[:3])
    zt = np.stack([np.r_[sr.so3_log(R0 @ tr.rodrigues(t * w)), z0[3:] + t * v] for t in ft])
    truth = np.concatenate([base.x_truth[:n0], zt.reshape(-1)])
    ds = sc.copy_of(base, num_frames=n_frames, frame_ids=np.arange(n_frames, dtype=np.int32),
                    obs_frame=np.repeat(np.arange(n_frames, dtype=np.int32), n), obs_cam=np.tile(base.obs_cam[sel], n_frames),
                    obs_marker=np.tile(base.obs_marker[sel], n_frames), obs_uv=np.zeros((n * n_frames, 8), dtype=np.float32),
                    x_truth=truth, x_full=np.concatenate([base.x_truth[:n0], np.tile(zt[0], n_frames)]))
    ds.obs_uv = pr.Reference(ds).projection(truth).astype(np.float32)
    empty = [0, n_frames // 2, n_frames - 1]
    return sc.without_frames(ds, empty), np.array(ds.x_full), zt, ft, empty, float(np.linalg.norm(w))
