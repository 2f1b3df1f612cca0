"""The data sets of the direct chain's certificates (tests/test_direct_certificate_host.py, tests/test_gpu_direct_certificates.py), by name --
TEST INFRASTRUCTURE ONLY.  Every builder returns a synthetic aar.Dataset; the shapes are the smallest at which the launch shape under test exists.

Rows of the device's reduced system: six per camera and marker, ROOTS INCLUDED (identity rows), cameras first -- so the root marker of a set
with C cameras sits at rows 6 C .. 6 C + 5, and the system has ceil(6 (C + M) / 96) tiles."""
import numpy as np

import aar


def tiles_of(ds, intrinsics=False):
    A = ds.num_cams + ds.num_markers + (ds.num_cams if intrinsics else 0)
    return -(-6 * A // 96)


def sweep_ds(nT):
    """16 nT - 3 entities (roots included), 24 frames: nT tiles, the last one 13/16 full (the sets of the SPCG certificates)"""
    n = 16 * nT - 3
    C = 3 if nT == 1 else 4
    return aar.synth(2, num_cams=C, num_markers=n - C, num_frames=24, min_view_cos=0.01, seed=1000 + nT)


def gauge_ds(cams, tiles):
    """`tiles` tiles with `cams` cameras: the root marker's rows start at row 6 cams"""
    return aar.synth(2, num_cams=cams, num_markers=16 * tiles - cams, num_frames=30, min_view_cos=0.01, seed=40 + cams + tiles)


def worklist_ds(frames=60):
    """two tiles (A = 24), `frames` frames"""
    return aar.synth(2, num_cams=4, num_markers=20, num_frames=frames, min_view_cos=0.01, seed=300 + frames)


def without_pairs(ds, unseen_marker, once_marker):
    """the set with every detection of one marker removed, and all but one frame's of another"""
    of, om = np.asarray(ds.obs_frame), np.asarray(ds.obs_marker)
    keep = om != unseen_marker
    fr = sorted(set(of[om == once_marker]))
    assert len(fr) >= 2
    keep &= ~((om == once_marker) & (of != fr[len(fr) // 2]))
    return ds.select_observations(keep)


def frame_entity_counts(ds, intrinsics=False):
    """per frame: the cameras + markers (+ intrinsics entities) seen in it -- the frame's slot count on the device"""
    of, oc, om = np.asarray(ds.obs_frame), np.asarray(ds.obs_cam), np.asarray(ds.obs_marker)
    out = []
    for f in range(ds.num_frames):
        s = of == f
        nc = len(set(oc[s]))
        out.append(nc * (2 if intrinsics else 1) + len(set(om[s])))
    return out


def frames_per_marker(ds):
    """per marker: the number of frames it is seen in"""
    of, om = np.asarray(ds.obs_frame), np.asarray(ds.obs_marker)
    return [len(set(of[om == m])) for m in range(ds.num_markers)]


def seen_entities(ds):
    return len(set(np.asarray(ds.obs_cam))) + len(set(np.asarray(ds.obs_marker)))


WIDE_TARGETS = [20, 29, 31, 45, 59, 61, 65, 70, 0, 0, 0, 0]      # entities per frame (0: all): both sides of 30 and of 60, and beyond 64


def wide_frames_ds(markers):
    """6 cameras and `markers` markers, every frame facing all of them, then cut down to WIDE_TARGETS entities per frame: frames of more than
    64 entities (k_schur<3>) beside frames that end inside its three prefetched passes of ten slots, and between them and 60"""
    ds = aar.synth(2, num_cams=6, num_markers=markers, num_frames=len(WIDE_TARGETS), min_view_cos=0.01, seed=500 + markers)
    of, om, oc = np.asarray(ds.obs_frame), np.asarray(ds.obs_marker), np.asarray(ds.obs_cam)
    keep = np.zeros(ds.num_obs, bool)
    for f, t in enumerate(WIDE_TARGETS):
        sel = of == f
        seen = sorted(set(om[sel]))
        if t:
            seen = seen[:t - len(set(oc[sel]))]
        keep |= sel & np.isin(om, seen)
    return ds.select_observations(keep)


def mfma_frames_ds(frames):
    """two tiles (A = 28), a handful of frames: the MFMA kernel's frame lists around SM_FPS and its two-deep ring"""
    return aar.synth(2, num_cams=4, num_markers=24, num_frames=frames, min_view_cos=0.01, seed=600 + frames)


def dense_count_ds(entities):
    """`entities` cameras + markers, all seen: the MFMA kernel's dense count is entities + 1 (the pseudo entity g_f)"""
    return aar.synth(2, num_cams=4, num_markers=entities - 4, num_frames=16, min_view_cos=0.01, seed=700 + entities)
