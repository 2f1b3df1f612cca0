"""Inputs of the sigma-fit tests (tests/test_smooth_fit_host.py, tests/test_gpu_smooth_fit.py) -- TEST INFRASTRUCTURE ONLY.

Built on tests/smooth_cases.py (imported, not edited): its emptied frames, its static object, and a random-walk sequence with known noise levels.
"""
import numpy as np

import aar
import projection_reference as pr
import smooth_cases as sc
import track_restated as tr

SROT, STRANS = 0.05, 0.02      # the start values the documents use
WALK_SIGMAS = (0.7, 0.03, 0.015)   # (sigma_px, sigma_rot, sigma_trans) of the recovery sequences: px, rad and metre per sqrt(frame)
WALK_FRAMES = 400
# Recovery caps, relative, per sigma (px, rot, trans): twice the worst deviation of the restated fit (tests/smooth_fit_restated.py, defaults, from
# SROT / STRANS) over the 20 sequences random_walk(WALK_FRAMES, *WALK_SIGMAS, seed) for seed = 100 .. 119, measured on the CPU: 1.184 % (seed
# 103), 3.429 % (seed 118), 3.801 % (seed 107).  DESIGN.md section 29 has the table.  (The sampling error of a sigma from 3 x 399 increments
# alone is 1 / sqrt(2 x 1197) = 2.0 %.)
CAPS = (2 * 0.01184, 2 * 0.03429, 2 * 0.03801)
assert max(CAPS) <= 0.25
WALK_SEEDS = (100, 101, 102)


def gaps(F):
    """frame times with a hole of five every seventh frame"""
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(F - 1) % 7 == 3) * 4.0])


def rel_motion(F, seed=3):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(max(F - 1, 0), 6)) * [0.05, 0.05, 0.05, 0.02, 0.02, 0.02]


def shape_dataset(F):
    """config 2 (3 above 65 frames, 4 above 127) at F frames with smooth_cases.emptied(F) emptied"""
    cfg = 2 if F <= 65 else 3 if F <= 127 else 4
    ds = aar.synth(cfg, num_frames=F)
    return sc.without_frames(ds, sc.emptied(F))


def parent_cases():
    """the three cases of tests/golden/smooth_fit_parent.npz: (name, ds, x0, frame_time, rel_motion)"""
    out = []
    ds = aar.synth(2, num_frames=17)
    out.append(("plain17", ds, sc.track_start(ds), None, None))
    ds = shape_dataset(65)
    out.append(("emptied65_gaps", ds, sc.track_start(ds), gaps(65), None))
    ds, x0, _ = sc.static_object(64)
    out.append(("static64_rel", ds, x0, None, rel_motion(64) * 0.1))
    return out


def parent_record(p, x0, ft, rel):
    """what the golden file holds per case, from one open problem: aar_track_smooth's outputs and aar_track_smooth_covariance's at its result"""
    xs, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, frame_time=ft, rel_motion=rel)
    S, R, crep = p.track_smooth_covariance(xs, SROT, STRANS, frame_time=ft, rel_motion=rel)
    skeys = [k for k in sorted(rep) if k != "seconds"]
    ckeys = [k for k in sorted(crep) if k != "seconds"]
    return dict(x=xs, frame_err=fe, pair_err=pe, report=np.array([float(rep[k]) for k in skeys]), S=S, R=R,
                cov_report=np.array([float(crep[k]) for k in ckeys]))


def parent_write(path):
    """records the golden file (run at the parent commit, on the GPU, with automatic-ar_amd and tests on the path)"""
    out = {}
    for name, ds, x0, ft, rel in parent_cases():
        with aar.Problem(ds) as p:
            for k, v in parent_record(p, x0, ft, rel).items():
                out["%s.%s" % (name, k)] = v
    np.savez_compressed(path, **out)


def walk(seed):
    """(ds, x0) of a recovery sequence"""
    return random_walk(WALK_FRAMES, *WALK_SIGMAS, seed=seed)


def expm_so3(w):
    return tr.rodrigues(np.asarray(w, dtype=np.float64))


def random_walk(F, sigma_px, sigma_rot, sigma_trans, seed, config=2):
    """A sequence whose object pose is a random walk: the camera, marker and observation index lists of the config's best-observed frame
    replicated F times (as smooth_cases.static_object), frame f + 1 = frame f with a right-multiplied Exp(N(0, sigma_rot^2 I)) and a
    translation step N(0, sigma_trans^2 I) -- the model of the between factor -- the corners projected through tests/projection_reference.py
    plus N(0, sigma_px) noise.  Returns (ds, x0) with x0 = cameras and markers at the truth, every frame at its true pose."""
    import smooth_restated as sr
    base = aar.synth(config)
    cnt = np.bincount(base.obs_frame, minlength=base.num_frames)
    f0 = int(cnt.argmax())
    sel = np.nonzero(base.obs_frame == f0)[0]
    n = len(sel)
    n0 = sc.ns(base)
    rng = np.random.default_rng(seed)
    z = np.zeros((F, 6))
    z[0] = base.x_truth[n0 + 6 * f0: n0 + 6 * f0 + 6]
    R = expm_so3(z[0, :3])
    for f in range(1, F):
        R = R @ expm_so3(rng.normal(0.0, sigma_rot, 3))
        z[f, :3] = sr.so3_log(R)
        z[f, 3:] = z[f - 1, 3:] + rng.normal(0.0, sigma_trans, 3)
    truth = np.concatenate([base.x_truth[:n0], z.reshape(-1)])
    ds = sc.copy_of(base, num_frames=F, frame_ids=np.arange(F, dtype=np.int32),
                    obs_frame=np.repeat(np.arange(F, dtype=np.int32), n), obs_cam=np.tile(base.obs_cam[sel], F),
                    obs_marker=np.tile(base.obs_marker[sel], F), obs_uv=np.zeros((n * F, 8), dtype=np.float32),
                    x_truth=truth, x_full=np.array(truth))
    uv = pr.Reference(ds).projection(truth)
    ds.obs_uv = (uv + rng.normal(0.0, sigma_px, size=uv.shape)).astype(np.float32)
    return ds, np.array(truth)
