"""Inputs of the smoothed-tracking tests (tests/test_smooth_restated_host.py, tests/test_gpu_track_smooth.py) -- TEST INFRASTRUCTURE ONLY."""
import numpy as np

import aar
import projection_reference as pr


def ns(ds):
    return 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)


def track_start(ds):
    """cameras / markers at the truth, the frame poses at the data set's perturbed start (as tests/test_gpu_track.py)"""
    x0 = np.array(ds.x_full)
    x0[:ns(ds)] = ds.x_truth[:ns(ds)]
    return x0


def copy_of(ds, **over):
    out = aar.Dataset.__new__(aar.Dataset)
    out.__dict__.update(ds.__dict__)
    out.__dict__.pop("_keep", None)
    for k, v in over.items():
        setattr(out, k, v)
    out.num_obs = len(out.obs_frame)
    return out


def without_frames(ds, frames):
    """the data set with every detection of the given frames removed (the frames stay)"""
    keep = ~np.isin(np.asarray(ds.obs_frame), np.asarray(list(frames)))
    return copy_of(ds, obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep], obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep])


def emptied(F):
    """frames of an F-frame problem to empty: the first, the last and a run of ten (what fits)"""
    s = {0, F - 1} | set(range(F // 3, min(F // 3 + 10, F))) if F >= 30 else ({0, F - 1} if F >= 4 else set())
    return sorted(s)


def static_object(n_frames=64, noise_px=0.3, seed=2024, config=2):
    """A static object: the best-observed frame of the config's truth, its observation list replicated n_frames times with fresh
    N(0, noise_px) corner noise, projected through tests/projection_reference.py.  Returns (ds, x0, truth pose [6]): cameras and markers
    at the truth, every frame started at that frame's perturbed pose of the config."""
    base = aar.synth(config)
    cnt = np.bincount(base.obs_frame, minlength=base.num_frames)
    f0 = int(cnt.argmax())
    sel = np.nonzero(base.obs_frame == f0)[0]
    n = len(sel)
    n0 = ns(base)
    zt = np.array(base.x_truth[n0 + 6 * f0: n0 + 6 * f0 + 6])
    zs = np.array(base.x_full[n0 + 6 * f0: n0 + 6 * f0 + 6])
    truth = np.concatenate([base.x_truth[:n0], np.tile(zt, n_frames)])
    ds = copy_of(base, num_frames=n_frames, frame_ids=np.arange(n_frames, dtype=np.int32),
                 obs_frame=np.repeat(np.arange(n_frames, dtype=np.int32), n), obs_cam=np.tile(base.obs_cam[sel], n_frames),
                 obs_marker=np.tile(base.obs_marker[sel], n_frames), obs_uv=np.zeros((n * n_frames, 8), dtype=np.float32),
                 x_truth=truth, x_full=np.concatenate([base.x_truth[:n0], np.tile(zs, n_frames)]))
    uv = pr.Reference(ds).projection(truth)
    rng = np.random.default_rng(seed)
    ds.obs_uv = (uv + rng.normal(0.0, noise_px, size=uv.shape)).astype(np.float32)
    return ds, np.array(ds.x_full), zt


def pose_rms(x, ds, zt):
    """RMS over the frames of |z_f - zt| (all six entries) -- the same measure for every method compared"""
    z = np.asarray(x)[ns(ds): ns(ds) + 6 * ds.num_frames].reshape(-1, 6)
    return float(np.sqrt(np.mean(np.sum((z - zt) ** 2, axis=1))))
