"""Inputs of the raw-detection live tracker tests (tests/test_live_detections_host.py, tests/test_gpu_live_detections.py) -- TEST INFRASTRUCTURE ONLY.

The scene is the synthetic generator's config 3 cut down to 4 cameras, 8 markers and 12 frames at 0.2 px, with markers accepted up to a slant of
acos 0.3 so that every frame has about ten detections in all four cameras (at the generator's default slant two markers are seen).
"""
import functools
from types import SimpleNamespace

import numpy as np

import aar
import oracle_lib as O
import smooth_cases as sc
import track_restated as tr
from test_initializer import DIST8, detections_of, poses_of, rigid, truth_transforms

FRAMES = 12


@functools.lru_cache(maxsize=None)
def case(distorted=False, seed=None):
    over = dict(num_cams=4, num_markers=8, num_frames=FRAMES, noise_px=0.2, min_view_cos=0.3)
    if seed is not None:
        over["seed"] = seed
    ds = aar.synth(3, **over)
    K = ds.cam_mats.reshape(-1, 3, 3)
    dists = [DIST8 * (1 + 0.1 * c) for c in range(ds.num_cams)] if distorted else [np.zeros(5)] * ds.num_cams
    det = detections_of(ds, dists if distorted else None)
    sol = sc.copy_of(ds, x_full=ds.x_truth.copy())       # the solved map: the ground truth, as test_track_app_flow_initial_object_poses_then_track
    cam, mk, fr = truth_transforms(ds)
    assert list(ds.cam_ids) == list(range(ds.num_cams)) and ds.num_frames == FRAMES
    frames = []
    for f in range(ds.num_frames):
        sel = det.det_frame == ds.frame_ids[f]
        frames.append((det.det_cam[sel].copy(), np.searchsorted(ds.marker_ids, det.det_id[sel]).astype(np.int32), det.det_uv[sel].copy()))
    return SimpleNamespace(ds=ds, K=K, dists=dists, det=det, sol=sol, ms=float(ds.marker_size), cam=np.array(cam), mk=np.array(mk), fr=np.array(fr),
                           frames=frames, ns=sc.ns(ds), distorted=distorted)


@functools.lru_cache(maxsize=None)
def oracle_object_poses(distorted=False):
    """the CPU yardstick: the oracle's Initializer with the map's transforms fixed -> (frame ids, object poses [F, 6])"""
    c = case(distorted)
    r = O.init_run(c.det.num_cams, c.det.num_frames, c.det.det_frame, c.det.det_cam, c.det.det_id, c.det.det_uv, c.ms, c.K, c.dists,
                   fixed=(c.ds.cam_ids, c.cam, c.ds.marker_ids, c.mk))
    return r["frame_ids"], r["T_object"], poses_of(r["T_object"]).reshape(-1, 6)


def root_only_detection(c, n=1):
    """n detections of the root marker by the root camera (identity transforms on both sides): the marker 2 m in front, turned to face the camera"""
    h = c.ms / 2
    X = np.array([[-h, h, 0], [h, h, 0], [h, -h, 0], [-h, -h, 0.0]])
    out = []
    for i in range(n):
        T = rigid(np.array([np.pi - 0.2 - 0.05 * i, 0.1, 0.05, 0.02 * i, -0.03, 2.0]))
        p = (c.K[c.ds.root_cam] @ (T[:3, :3] @ X.T + T[:3, 3:4])).T
        out.append((p[:, :2] / p[:, 2:3]).reshape(8))
    return (np.full(n, c.ds.root_cam, dtype=np.int32), np.full(n, c.ds.root_marker, dtype=np.int32), np.array(out, dtype=np.float32))


def pooled(c, n):
    """n detections drawn from all frames of the scene in turn (they disagree on the object pose: only the vote's arithmetic is of interest)"""
    cam = np.concatenate([f[0] for f in c.frames]); mk = np.concatenate([f[1] for f in c.frames]); uv = np.concatenate([f[2] for f in c.frames])
    idx = np.arange(n) % len(cam)
    return cam[idx], mk[idx], uv[idx]


def frame_data(c, cam, mk, uv):
    """track_restated's per-frame dict for one pushed frame (corners already undistorted)"""
    n = len(cam)
    one = sc.copy_of(c.sol, num_frames=1, obs_frame=np.zeros(n, dtype=np.int32), obs_cam=np.asarray(cam), obs_marker=np.asarray(mk),
                     obs_uv=np.asarray(uv, dtype=np.float32).reshape(-1, 8))
    x = np.r_[c.sol.x_full[:c.ns], np.zeros(6)]
    return tr.TrackData(one, x).frame(0)


def project(c, cam, mk, z, noise=0.0, rng=None):
    """the corners [n, 8] of the detections (cam, mk) with the object at pose z, as float32"""
    fd = frame_data(c, cam, mk, np.zeros((len(cam), 8)))
    uv = -tr.residuals(fd, np.asarray(z, dtype=np.float64)).reshape(-1, 8)
    if noise:
        uv = uv + rng.normal(0, noise, uv.shape)
    return uv.astype(np.float32)
