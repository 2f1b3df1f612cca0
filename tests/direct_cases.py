"""The data sets of the direct chain's certificates (tests/test_direct_certificate_host.py, tests/test_gpu_direct_certificates.py, and the runs of
tests/test_direct_run_certificate_host.py, tests/test_gpu_speculative_path.py), by name --
TEST INFRASTRUCTURE ONLY.  Every builder returns a synthetic aar.Dataset; the shapes are the smallest at which the launch shape under test exists.

Rows of the device's reduced system: six per camera and marker, ROOTS INCLUDED (identity rows), cameras first -- so the root marker of a set
with C cameras sits at rows 6 C .. 6 C + 5, and the system has ceil(6 (C + M) / 96) tiles."""
import itertools
import threading

import numpy as np

import aar
from pair_priors_restated import pose_of
from reduced_system import rodrigues, slot_col, so3_log


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


def ldl_env(monkeypatch, fused=3, lookahead=1, bs_rides=1):
    monkeypatch.setenv("AAR_FUSED_PANEL", str(fused))
    monkeypatch.setenv("AAR_LDL_LOOKAHEAD", str(lookahead))
    monkeypatch.setenv("AAR_BS_RIDES", str(bs_rides))


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


# ---- the LM runs of the speculative path (tests/test_direct_run_certificate_host.py finds on the CPU that every one offers its predicted steps;
# tests/test_gpu_speculative_path.py runs them on the device) ----
def passa_cut_ds():
    """two tiles, 24 frames, five of them cut down to SMALL_TARGETS slots: frames with fewer slots than a wavefront has lanes"""
    return cut_frames(worklist_ds(24), SMALL_TARGETS)[0]


def sparse_view_ds():
    """two tiles, 24 frames, markers seen only close to head-on: between 15 and 30 observations per frame"""
    return aar.synth(2, num_cams=4, num_markers=20, num_frames=24, min_view_cos=0.5, seed=324)


def far_start_ds():
    """config 2 cut to 40 frames, started twenty times as far from the solution as the default: with tau = 1e-6 its run has rejected tries,
    accepted steps with a gain below 0.94 and predicted steps (the set of test_steps_of_a_run_with_rejected_tries)"""
    return aar.synth(2, num_frames=40, init_scale=20.0)


def fixed_entities(ds):
    fc = [c for c in range(ds.num_cams) if c != ds.root_cam][:2]
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker][3:4]
    return dict(fixed_cams=fc, fixed_markers=fm)


def camera_priors(ds, x):
    """a pose prior on every camera but the root, near its pose at x"""
    rng = np.random.default_rng(3)
    pr = []
    for c in range(ds.num_cams):
        if c != ds.root_cam:
            col = slot_col(ds, "camera", c)
            A = rng.standard_normal((6, 6))
            pr.append(("camera", c, x[col:col + 6] + np.r_[0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)], 1e3 * (A @ A.T + 6 * np.eye(6))))
    return pr


def marker_pair_priors(ds, x, n=6):
    """relative pose priors between n pairs of neighbouring markers (one with a root end), near their relative poses at x"""
    rng = np.random.default_rng(5)
    free = [m for m in range(ds.num_markers) if m != ds.root_marker]
    ends = [(ds.root_marker, free[0])] + [(free[2 * i + 1], free[2 * i + 2]) for i in range(n - 1)]
    out = []
    for a, b in ends:
        xa, xb = pose_of(ds, x, "marker", a), pose_of(ds, x, "marker", b)
        Ra, Rb = rodrigues(xa[:3]), rodrigues(xb[:3])
        u = rng.standard_normal(3)
        Rrel = Ra.T @ Rb @ rodrigues(0.02 * u / np.linalg.norm(u)).T
        A = rng.standard_normal((6, 6))
        out.append(("marker", a, b, np.r_[so3_log(Rrel), Ra.T @ (xb[3:] - xa[3:]) + 0.02 * rng.standard_normal(3)], 1e2 * (A @ A.T + 6 * np.eye(6))))
    return out


def _golden(name):
    from conftest import load_golden
    return load_golden(name)[0]


# name -> (data set, Problem options beside solver [priors / pair_priors / fixed as the strings the callers resolve], tau, predicted steps the run
# must offer among its first ten)
SPEC_RUNS = {
    "passa_cut": (passa_cut_ds, {}, 1.0, 3), "avg_le_14": (lambda: sweep_ds(1), {}, 1.0, 3), "avg_15_30": (sparse_view_ds, {}, 1.0, 3),
    "avg_31_96": (lambda: worklist_ds(24), {}, 1.0, 3), "avg_gt_96": (lambda: sweep_ds(5), {}, 1.0, 3),
    "wide_84": (lambda: wide_frames_ds(84), {}, 1.0, 3), "worklist_F60": (lambda: worklist_ds(60), {}, 1.0, 3),
    "huber": (lambda: _golden("g1_cfg2_huber"), dict(with_huber=True, huber_delta=2.5), 1.0, 3),
    "intrinsics": (lambda: _golden("g1_cfg2_intr"), dict(intrinsics=True), 1.0, 3),
    "priors": (lambda: _golden("g1_cfg3_cut"), dict(priors="camera", pair_priors="marker"), 1.0, 3),
    "fixed": (lambda: gauge_ds(16, 3), dict(fixed=True), 1.0, 3),
    "cams_off": (lambda: gauge_ds(16, 3), dict(optimize=(False, True, True)), 1.0, 3),
    "markers_off": (lambda: gauge_ds(16, 3), dict(optimize=(True, False, True)), 1.0, 3),
    "frames_off": (lambda: gauge_ds(16, 3), dict(optimize=(True, True, False)), 1.0, 3),
    "sweep1": (lambda: sweep_ds(1), {}, 1.0, 3), "sweep2": (lambda: sweep_ds(2), {}, 1.0, 3), "sweep3": (lambda: sweep_ds(3), {}, 1.0, 3),
    "sweep5": (lambda: sweep_ds(5), {}, 1.0, 3),
    "far_start": (far_start_ds, {}, 1e-6, 3),
}
for _F in (1, 2, 3, 5, 9):
    SPEC_RUNS["mfma_F%d" % _F] = (lambda F=_F: mfma_frames_ds(F), {}, 1.0, 3)
for _e in (30, 31, 32):
    SPEC_RUNS["dense_%d" % (_e + 1)] = (lambda e=_e: dense_count_ds(e), {}, 1.0, 3)


def spec_run(name):
    """(ds, x0, Problem keyword arguments, tau, minimum of predicted steps, huber delta or None) of a named run"""
    make, opts, tau, need = SPEC_RUNS[name]
    ds = make()
    kw = dict(opts)
    x = np.asarray(ds.x_full, dtype=np.float64)
    huber = kw.pop("huber_delta", None)
    if kw.pop("fixed", False):
        kw.update(fixed_entities(ds))
    if kw.get("priors") == "camera":
        kw["priors"] = camera_priors(ds, x)
    if kw.get("pair_priors") == "marker":
        kw["pair_priors"] = marker_pair_priors(ds, x)
    if kw.get("intrinsics"):
        K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 9)
        d = np.asarray(ds.dist_coeffs, dtype=np.float64).reshape(-1, 5)
        x = np.concatenate([x, np.concatenate([np.stack([K[:, 0], K[:, 2], K[:, 4], K[:, 5]], axis=1), d], axis=1).reshape(-1)])
    return ds, x, kw, tau, need, huber
