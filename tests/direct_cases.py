"""The data sets of the direct chain's certificates (tests/test_direct_certificate_host.py, tests/test_gpu_direct_certificates.py), by name --
TEST INFRASTRUCTURE ONLY.  Every builder returns a synthetic aar.Dataset; the shapes are the smallest at which the launch shape under test exists.

Rows of the device's reduced system: six per camera and marker, ROOTS INCLUDED (identity rows), cameras first -- so the root marker of a set
with C cameras sits at rows 6 C .. 6 C + 5, and the system has ceil(6 (C + M) / 96) tiles."""
import itertools
import threading

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


SMALL_TARGETS = [2, 3, 10, 11, 12]                 # slots per frame: 3, 6, 55, 66, 78 slot pairs -- both sides of one round of 64 lanes
SMALL_TARGETS_INTRINSICS = [3, 6, 10, 11, 12]      # (a camera brings its intrinsics entity: one camera and one marker are three slots)


def cut_frames(ds, targets, intrinsics=False):
    """(ds with one frame per target cut down to that many slots -- cameras [+ their intrinsics entities] + markers --, those frames): every
    target takes the first frame not yet used that can be cut to it, with as many of its cameras as fit and the first markers that all of them see"""
    of, oc, om = np.asarray(ds.obs_frame), np.asarray(ds.obs_cam), np.asarray(ds.obs_marker)
    cw = 2 if intrinsics else 1
    cut = {}
    for t in targets:
        for f in (f for f in range(ds.num_frames) if f not in cut):
            sel = of == f
            cams = sorted(set(oc[sel]))
            for pick in (c for nc in range(min(len(cams), (t - 1) // cw), 0, -1) for c in itertools.combinations(cams, nc)):
                sc = sel & np.isin(oc, pick)
                for mk in itertools.islice(itertools.combinations(sorted(set(om[sc])), t - cw * len(pick)), 500):
                    k = sc & np.isin(om, mk)
                    if cw * len(set(oc[k])) + len(set(om[k])) == t:
                        cut[f] = k
                        break
                if f in cut:
                    break
            if f in cut:
                break
        else:
            raise ValueError("no frame can be cut to %d slots" % t)
    keep = ~np.isin(of, list(cut))
    for k in cut.values():
        keep |= k
    return ds.select_observations(keep), list(cut)


def small_frames_ds():
    """4 cameras and 12 markers, every frame facing all of them, the first five cut down to SMALL_TARGETS slots (k_cov_frames: fewer slot pairs
    than lanes, and the first pairs of a second round)"""
    ds = aar.synth(2, num_cams=4, num_markers=12, num_frames=16, min_view_cos=0.01, seed=800)
    return cut_frames(ds, SMALL_TARGETS)[0]


def without_frame(ds, f):
    """the set with every detection of frame f removed"""
    return ds.select_observations(np.asarray(ds.obs_frame) != f)


def roots_only_frame(ds):
    """(the set with one frame cut down to the root camera's detection of the root marker, that frame): its W blocks are all gauge rows"""
    of, oc, om = np.asarray(ds.obs_frame), np.asarray(ds.obs_cam), np.asarray(ds.obs_marker)
    root = (oc == ds.root_cam) & (om == ds.root_marker)
    f = int(of[root][len(of[root]) // 2])
    return ds.select_observations((of != f) | root), f


def mfma_frames_ds(frames):
    """two tiles (A = 28), a handful of frames: the MFMA kernel's frame lists around SM_FPS and its two-deep ring"""
    return aar.synth(2, num_cams=4, num_markers=24, num_frames=frames, min_view_cos=0.01, seed=600 + frames)


def dense_count_ds(entities):
    """`entities` cameras + markers, all seen: the MFMA kernel's dense count is entities + 1 (the pseudo entity g_f)"""
    return aar.synth(2, num_cams=4, num_markers=entities - 4, num_frames=16, min_view_cos=0.01, seed=700 + entities)


# ---- launch structures of the LDL^T chain and in-process ranks, shared by the GPU certificate modules ----
def ldl_expected(nT, fused, lookahead, bs_rides):
    """launches of one factorisation (launch_chol, solve_kernels.hip)"""
    panel = trsm = update = 0
    for s in range(nT):
        m = nT - s - 1
        if 0 < m <= fused:
            panel += 1
        elif m > 0:
            trsm += 1
            if not (lookahead and m >= 2):
                update += 1
    back = 1 if nT > 1 and not (bs_rides and nT <= 3) else 0
    return dict(k_ldl_diag=nT, k_ldl_panel=panel, k_ldl_trsm=trsm, k_ldl_update=update, k_ldl_backsolve=back)


def ldl_env(monkeypatch, fused=3, lookahead=1, bs_rides=1, backsub_rides=0):
    monkeypatch.setenv("AAR_FUSED_PANEL", str(fused))
    monkeypatch.setenv("AAR_LDL_LOOKAHEAD", str(lookahead))
    monkeypatch.setenv("AAR_BS_RIDES", str(bs_rides))
    monkeypatch.setenv("AAR_BACKSUB_RIDES", str(backsub_rides))


def run_ranks(world, fn):
    grp = aar.LocalGroup(world)
    out, errs = [None] * world, []

    def run(rank):
        try:
            comm = aar.Comm.local(grp, rank)
            try:
                out[rank] = fn(comm, rank)
            finally:
                comm.close()
        except Exception as e:      # noqa: BLE001
            errs.append((rank, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    grp.close()
    assert not errs, errs
    return out
