"""Inputs of the marginalised-anchor / covariance tests of the live tracker (tests/test_live_marginal_host.py, tests/test_gpu_live_marginal.py)
-- TEST INFRASTRUCTURE ONLY.  The stream cases are built as tests/test_gpu_live_tracker.py builds its own (push times with holes, a pose_init on
two pushes of three) on the scene of tests/live_detection_cases.py (4 cameras, 8 markers, about ten detections per frame); the restated runs are computed once per case and shared."""
import functools
from types import SimpleNamespace

import numpy as np

import aar
import live_marginal_restated as lm
import projection_reference as pr
import smooth_cases as sc
import track_restated as tr

SROT, STRANS = 0.05, 0.02      # as tests/test_gpu_live_tracker.py
N = 20                         # pushes: a lag-15 ring wraps

# the batch property (moving_object): sigmas found on the CPU -- tight enough that frames behind the window still pull on it
BATCH_SROT, BATCH_STRANS, BATCH_LAG, BATCH_FRAMES = 2e-3, 1e-3, 3, 24


def times(n):
    """push times with a hole of five every seventh frame"""
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(n - 1) % 7 == 3) * 4.0])


def keep_first(ds, counts):
    """the data set with only the first counts[f] detections of frame f (None: all)"""
    keep = np.ones(ds.num_obs, dtype=bool)
    for f, c in enumerate(counts):
        idx = np.nonzero(np.asarray(ds.obs_frame) == f)[0]
        if c is not None:
            keep[idx[c:]] = False
    return sc.copy_of(ds, obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep], obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep])


def frame_obs(ds, f):
    sel = np.asarray(ds.obs_frame) == f
    return ds.obs_cam[sel], ds.obs_marker[sel], ds.obs_uv[sel]


# detections kept per frame in the "counts" cases: frames with 0 and 1 detections inside the stream, and every ring slot of lag 1 / 3 (2 / 4
# slots) reused by a frame with fewer and by one with more
COUNTS = [None, None, 3, None, 2, 0, None, 1, 3, None, None, 2, None, 4, 1, None, None, 0, 2, None]


@functools.lru_cache(maxsize=None)
def case(kind, lag, smooth=True, first_empty=False):
    """kind: "counts" | "huber" | "far" | "plain"; first_empty: the first frame has no detections (the empty stream start)"""
    delta, lmkw, scale, every_init, n = None, {}, 1.0, False, N
    if kind == "far":
        scale, lmkw, every_init, n = 20.0, dict(tau=1e-6), True, 24      # (24 frames: the ones with rejected tries lie behind the 20th)
    if kind == "far":
        ds = aar.synth(2, num_frames=n, init_scale=scale)       # tests/test_gpu_live_tracker.py's far start: the one with rejected tries
    else:
        ds = aar.synth(3, num_cams=4, num_markers=8, num_frames=n, noise_px=0.2, min_view_cos=0.3)     # tests/live_detection_cases.py's scene
    x0 = sc.track_start(ds)
    if kind == "counts":
        ds = keep_first(ds, COUNTS)
    if kind == "huber":
        delta = 0.5
        uv = np.array(ds.obs_uv)
        rng = np.random.default_rng(11)
        hit = rng.choice(len(uv), size=len(uv) // 8, replace=False)
        uv[hit, rng.integers(0, 8, size=len(hit))] += 50.0                  # 50 px outliers
        ds = sc.copy_of(ds, obs_uv=uv.astype(np.float32))
    if first_empty:
        ds = keep_first(ds, [0] + [None] * (n - 1))
    td = tr.TrackData(ds, x0)
    has_init = [True if every_init else (f % 3 != 1) for f in range(n)]
    kw = dict(lag=lag, smooth=smooth, with_huber=delta is not None, max_obs_per_frame=int(max(np.bincount(ds.obs_frame, minlength=n).max(), 1)))
    if smooth:
        kw.update(sigma_rot=SROT, sigma_trans=STRANS)
    if delta is not None:
        kw.update(huber_delta=delta)
    return SimpleNamespace(name="%s-lag%d%s" % (kind, lag, "" if smooth else "-track"), ds=ds, x0=x0, td=td, n=n, lag=lag, smooth=smooth,
                           times=times(n), delta=delta, lm=lmkw, kw=kw, has_init=has_init, sol=sc.copy_of(ds, x_full=x0))


@functools.lru_cache(maxsize=None)
def restated(kind, lag, anchor, smooth=True, first_empty=False):
    """every push of the case by live_marginal_restated.LiveM (each dict also carries window and anchor after the push)"""
    c = case(kind, lag, smooth, first_empty)
    live = lm.LiveM(c.td, lag=c.lag, smooth=c.smooth, sigma_rot=SROT, sigma_trans=STRANS, delta=-1.0 if c.delta is None else c.delta,
                    anchor=anchor, **c.lm)
    out = []
    for f in range(c.n):
        r = live.push(f, c.times[f], pose_init=c.td.z0[f] if c.has_init[f] else None)
        r["window"], r["anchor"] = live.window()
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def moving_object(n_frames=BATCH_FRAMES, noise_px=0.5, seed=7, config=2):
    """A slowly moving object: the best-observed frame of the config's truth carried along a gentle arc (about 2 mm and 0.1 degree per frame),
    its observation list replicated with fresh N(0, noise_px) corner noise.  Returns (ds, x0): cameras and markers at the truth, every frame
    started at the first frame's true pose."""
    base = aar.synth(config)
    cnt = np.bincount(base.obs_frame, minlength=base.num_frames)
    f0 = int(cnt.argmax())
    sel = np.nonzero(base.obs_frame == f0)[0]
    n = len(sel)
    n0 = sc.ns(base)
    zt = np.array(base.x_truth[n0 + 6 * f0: n0 + 6 * f0 + 6])
    k = np.arange(n_frames)[:, None]
    vel = np.array([1.5e-3, -1.0e-3, 0.8e-3, 2e-3, 1e-3, -1.5e-3])
    zs = zt[None, :] + k * vel[None, :] + 0.5 * (k / n_frames) ** 2 * np.array([0.0, 2e-3, 0.0, -4e-3, 0.0, 3e-3])[None, :]
    truth = np.concatenate([base.x_truth[:n0], zs.reshape(-1)])
    ds = sc.copy_of(base, num_frames=n_frames, frame_ids=np.arange(n_frames, dtype=np.int32),
                    obs_frame=np.repeat(np.arange(n_frames, dtype=np.int32), n), obs_cam=np.tile(base.obs_cam[sel], n_frames),
                    obs_marker=np.tile(base.obs_marker[sel], n_frames), obs_uv=np.zeros((n * n_frames, 8), dtype=np.float32),
                    x_truth=truth, x_full=np.concatenate([base.x_truth[:n0], np.tile(zt, n_frames)]))
    uv = pr.Reference(ds).projection(truth)
    rng = np.random.default_rng(seed)
    ds.obs_uv = (uv + rng.normal(0.0, noise_px, size=uv.shape)).astype(np.float32)
    return ds, np.array(ds.x_full)
