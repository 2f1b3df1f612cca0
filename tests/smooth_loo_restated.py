"""Float64 restatement of the per-detection layer of a smoothed track (aar_track_smooth_detection_leverage, _detection_loo, _predict_corners,
_gate_detections) -- TEST INFRASTRUCTURE ONLY, numpy only.

It stands on tests/smooth_restated.py / tests/smooth_cv_restated.py (the dense H of either motion model, complex-step prior Jacobians),
tests/projection_reference.py (the forward model, G = du / dz_f by the complex step through tests/predict_restated.query_projection) and
tests/loo_restated.py (`tail`, `statistics`, and LooSystem for the exact identities).

    C_i = G_i Sigma_ff G_i^T,   Sigma = H^-1,   H_p = H - blockdiag(V_f),  V_f = sum over the frame's detections of G_i^T G_i
    sum_i tr(C_i) = tr(Sigma blockdiag(V)) = tr(Sigma (H - H_p)) = 6 F - tr(Sigma H_p)                       (no Huber weights)

The linear problem behind the identities is LooSystem's with the frame poses as the only unknowns and the motion prior as the quadratic term
H_p: cost(d) = |r - G d|^2 + d^T H_p d.  `fault` plants the mistakes this layer can make:

    "no_prior"   Sigma_ff replaced by V_f^-1 (the prior forgotten)
    "lag_block"  the lag-one block Sigma_{f,f+1} (Sigma_{f-1,f} for the last frame) taken for the diagonal one
    "huber_g"    G scaled by the corners' Huber weights (the smoother's weighted Jacobian taken for the unweighted one)
    "c_sign", "nu"   loo_restated's, passed through to its tail / statistics
"""
import numpy as np

import loo_restated as lr
import predict_restated as prs
import projection_reference as pr
import smooth_cases as sc
import smooth_cv_restated as cv
import smooth_restated as sr
import track_restated as tr

FAULTS = ("no_prior", "lag_block", "huber_g", "c_sign", "nu")
U53 = 2.0 ** -53
FLAT_BAR = prs.FLAT_BAR


def frames_of(ds, x):
    n0 = sc.ns(ds)
    return np.asarray(x, dtype=np.float64)[n0:n0 + 6 * ds.num_frames].reshape(ds.num_frames, 6)


def with_frames(ds, x, z):
    out = np.array(x, dtype=np.float64)
    n0 = sc.ns(ds)
    out[n0:n0 + 6 * ds.num_frames] = np.asarray(z).reshape(-1)
    return out


def problem(ds, x, sigma_rot, sigma_trans, model="rw", sigma_rot0=0.0, sigma_trans0=0.0, frame_time=None, rel_motion=None, delta=None):
    """the restated smoother of either model over ds at x"""
    td = tr.TrackData(ds, x)
    if model == "cv":
        return cv.SmoothCvProblem(td, sigma_rot, sigma_trans, sigma_rot0, sigma_trans0, delta=delta, frame_time=frame_time)
    return sr.SmoothProblem(td, sigma_rot, sigma_trans, delta=delta, frame_time=frame_time, rel_motion=rel_motion)


def dense_system(sp, z):
    """(H [6F, 6F] at mu = 0, (data cost, prior cost)) of the restated smoother at z [F, 6]"""
    blocks = sp.system(z)
    H = cv.dense(*blocks[:3]) if isinstance(sp, cv.SmoothCvProblem) else sr.dense(*blocks[:2])
    Ef, Pe = sp.costs(z)
    return H, (float(np.sum(Ef)), float(np.sum(Pe)))


def converged(sp, z0, **lm):
    """the restated LM of the model to its stopping rule from z0"""
    run = cv.smooth_lm if isinstance(sp, cv.SmoothCvProblem) else sr.smooth_lm
    return run(sp, z0, **lm)


class TrackSystem:
    """What LooSystem asks of a PredictSystem, for a smoothed track: the frame poses are the only unknowns, column 6 f + k"""

    def __init__(self, ds):
        self.ds = ds
        self.num_live_vars = 6 * int(ds.num_frames)
        self.idx = np.arange(self.num_live_vars)
        self.pos = {int(k): int(k) for k in self.idx}

    def z_columns(self, c, m, f):
        col = np.full(18, -1, dtype=np.int64)
        col[12:18] = 6 * f + np.arange(6)
        return col


def corners_at(ds, x, cams, markers, poses):
    """(uv [Q, 8], G [Q, 8, 6] = du / d(pose) by the complex step, depth [Q, 4]) of (camera index, marker index) at the poses [Q, 6]"""
    ref = pr.Reference(ds)
    cam, mk, _ = ref.entity_vectors(np.asarray(x, dtype=np.float64))
    cams, markers = np.asarray(cams, dtype=np.int64).reshape(-1), np.asarray(markers, dtype=np.int64).reshape(-1)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 6)
    K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 3, 3)[cams]
    pc, pm = cam[cams], mk[markers]
    uv = pr.project(pc, pm, poses, K, ref.h)
    depth = pr.camera_points(pc, pm, poses, ref.h)[..., 2]
    G = np.empty((len(cams), 8, 6))
    for k in range(6):
        a = poses.astype(np.complex128)
        a[:, k] += 1j * pr.CSTEP
        G[:, :, k] = pr.project(pc.astype(np.complex128), pm.astype(np.complex128), a, K.astype(np.complex128), ref.h).imag / pr.CSTEP
    return uv, G, depth


def push(G, S):
    """(C = G S G^T, s = | |G| |S| |G^T| |_F) over arrays G [n, 8, 6], S [n, 6, 6]"""
    C = np.einsum("nri,nij,nsj->nrs", G, S, G)
    s = np.linalg.norm(np.einsum("nri,nij,nsj->nrs", np.abs(G), np.abs(S), np.abs(G)), axis=(1, 2))
    return C, s


def certificate_bar(s):
    """(12 2^-53 + 2 SCALED_BAR) s: the two six-term products of the kernel, and the closed-form Jacobian against the complex step, which
    enters C twice -- predict_restated.certificate_bars without its slot terms"""
    return (12 * U53 + 2 * pr.SCALED_BAR) * np.asarray(s)


class SmoothLoo:
    """The layer at x: G, r, u of the problem's detections in reference order; H, its inverse and H_p; the costs and nu.

    H, cost: from `dense_system` (the restatement alone) or from the device's aar_track_smooth_system2.  frame_cov [F, 6, 6]: the
    device's own blocks to feed the certificate (default: the blocks of numpy.linalg.inv(H))."""

    def __init__(self, ds, x, H, cost, frame_cov=None, huber_delta=None):
        self.ds, self.x = ds, np.asarray(x, dtype=np.float64)
        F = self.F = int(ds.num_frames)
        self.q3 = prs.detection_queries(ds)
        self.N = len(self.q3)
        self.frame = self.q3[:, 2] if self.N else np.zeros(0, dtype=np.int64)
        z = frames_of(ds, x)
        self.uv, self.G, self.depth = corners_at(ds, x, self.q3[:, 0], self.q3[:, 1], z[self.frame]) if self.N else (np.zeros((0, 8)), np.zeros((0, 8, 6)), np.zeros((0, 4)))
        self.obs = np.asarray(ds.obs_uv, dtype=np.float32).reshape(-1, 8).astype(np.float64)
        self.r = self.obs - self.uv
        self.behind = ~(self.depth > 0).all(axis=1)
        self.H = np.asarray(H, dtype=np.float64)
        self.Sigma = np.linalg.inv(self.H)
        self.V = np.zeros((F, 6, 6))
        np.add.at(self.V, self.frame, np.einsum("nri,nrj->nij", self.G, self.G))
        self.Hp = self.H.copy()
        for f in range(F):
            self.Hp[6 * f:6 * f + 6, 6 * f:6 * f + 6] -= self.V[f]
        self.cost = float(cost[0] + cost[1])
        self.nu = 8 * self.N + 6 * max(F - 1, 0) - 6 * F
        self.sigma2 = self.cost / self.nu if self.nu > 0 else 0.0
        self.frame_cov = None if frame_cov is None else np.asarray(frame_cov, dtype=np.float64).reshape(F, 6, 6)
        self.huber_delta = huber_delta

    def block(self, a, b):
        return self.Sigma[6 * a:6 * a + 6, 6 * b:6 * b + 6]

    def sigma_ff(self, fault=None):
        """[F, 6, 6] the block each frame's detections are pushed through"""
        F = self.F
        if fault == "no_prior":
            out = np.full((F, 6, 6), np.nan)
            for f in range(F):
                if np.linalg.matrix_rank(self.V[f]) == 6:
                    out[f] = np.linalg.inv(self.V[f])
            return out
        if fault == "lag_block":
            return np.stack([self.block(f, f + 1) if f + 1 < F else self.block(f - 1, f) for f in range(F)])
        if self.frame_cov is not None:
            return self.frame_cov
        return np.stack([self.block(f, f) for f in range(F)])

    def all_C(self, fault=None):
        """(C [N, 8, 8], s [N])"""
        G = self.G
        if fault == "huber_g":
            e = (self.r.reshape(-1, 4, 2) ** 2).sum(axis=2)
            w = pr.huber_weight(e, self.huber_delta)
            G = G * np.repeat(w, 2, axis=1)[:, :, None]
        return push(G, self.sigma_ff(fault)[self.frame])

    def quantities(self, f_max=None, fault=None, C=None):
        """What aar_track_smooth_detection_loo returns, as a dict of arrays: loo_resid, q, F, cook, leverage, margin, status, keep"""
        if C is None:
            C, _ = self.all_C(fault)
        C = np.where(self.behind[:, None, None], np.nan, C)
        w, q, k, mg, und = lr.tails(C, self.r, 3, fault)
        Fs, cook = lr.statistics(q, k, self.cost, self.nu, 6 * self.F, fault)
        lev = np.where(self.behind, np.nan, prs.trace_tree(C))
        st = (self.behind * 1 + und * lr.UNDETERMINED).astype(np.uint8)
        keep = np.ones(self.N, dtype=np.uint8)
        if f_max is not None:
            with np.errstate(invalid="ignore"):
                keep[(st == 0) & (Fs > f_max)] = 0
        return dict(loo_resid=w, q=q, F=Fs, cook=cook, leverage=lev, margin=mg, status=st, keep=keep, k=k)

    def leverage_identity(self, C=None):
        """(sum_i tr(C_i), 6 F - tr(Sigma H_p)): equal without Huber weights"""
        if C is None:
            C, _ = self.all_C()
        return float(np.trace(C, axis1=1, axis2=2).sum()), float(6 * self.F - np.trace(self.Sigma @ self.Hp))

    def loo_system(self):
        """loo_restated.LooSystem of the linear problem: the exact identities by routes that never form (I - C_i)^-1"""
        return lr.LooSystem(TrackSystem(self.ds), self.x, Hp=self.Hp)

    def det_err(self):
        """e_d of aar_problem_residual_report: sqrt(sum r^2 / 4) per detection"""
        return np.sqrt((self.r ** 2).sum(axis=1) / 4.0)


def gate(C, e):
    """(m2 [n], margin [n], undetermined [n]) of innovations e [n, 8] against C [n, 8, 8]: loo_restated's tail in mode 4"""
    _, q, _, mg, und = lr.tails(C, e, 4)
    return q, mg, und


# ---- the planted outlier (tests/test_smooth_loo_restated_host.py, tests/test_gpu_track_smooth_loo.py): smooth_cases.static_object with one
# frame thinned to two detections and the corners of the first of them shifted.  In a frame that thin the pose follows the shifted detection:
# its raw error after smoothing is ordinary, its F is not.
PLANT = dict(n_frames=12, noise_px=0.3, seed=2024, frame=5, keeps=2, offset=(3.0, 3.0), sigma_rot=0.01, sigma_trans=0.01)
PLANT_MODELS = {"rw": dict(model="rw"), "cv": dict(model="cv", sigma_rot0=1.0, sigma_trans0=1.0)}
PLANT_LM = dict(min_avg=0.0, max_iters=30)          # the restated LM run to the end of its progress, not to the default stopping rule
PLANT_F_MAX = lr.PLANT_F_MAX


def planted():
    """(ds, x0, index of the shifted detection)"""
    ds, x0, _ = sc.static_object(n_frames=PLANT["n_frames"], noise_px=PLANT["noise_px"], seed=PLANT["seed"])
    fr = np.asarray(ds.obs_frame)
    keep = np.ones(ds.num_obs, dtype=bool)
    inf = np.nonzero(fr == PLANT["frame"])[0]
    keep[inf[PLANT["keeps"]:]] = False
    ds = sc.copy_of(ds, obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep], obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep].copy())
    i = int(np.nonzero(np.asarray(ds.obs_frame) == PLANT["frame"])[0][0])
    ds.obs_uv[i] += np.tile(np.asarray(PLANT["offset"], dtype=np.float32), 4)
    return ds, x0, i


def ranks(values, i):
    """the rank of detection i by descending value (0 = first), NaN last"""
    v = np.where(np.isnan(values), -np.inf, values)
    return int((v > v[i]).sum())


# ---- the second-order gap of the linearisation (tests/test_smooth_loo_restated_host.py, tests/test_gpu_track_smooth_loo.py): q_i against an
# actual deletion of detection i and a re-smooth, on the planted case at its converged track, for loo_restated.three_detections.
# MEASURED in the restatement (restated LM with PLANT_LM): |drop - q| / q = 3.22e-4, 6.8e-5, 2.9e-5 under the random walk and 3.17e-4,
# 1.9e-5, 3.9e-5 under constant velocity; the constant is the worst of them, rounded up in its third digit.  The thin frame's two
# detections carry the large ones: deleting one of two leaves a frame that moves far.
GAP_Q = 3.23e-4


def without_detection(ds, i):
    keep = np.ones(ds.num_obs, dtype=bool)
    keep[i] = False
    return sc.copy_of(ds, obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep], obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep])
