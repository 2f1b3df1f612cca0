"""Independent float64 reference of the observation model and its derivative by the complex step.

TEST INFRASTRUCTURE ONLY (numpy): imported by tests/test_projection_reference_host.py and tests/test_gpu_observation_passes.py.

What the kernels of csrc/eval_kernels.hip and oracle/ba_oracle.cpp share is the CLOSED FORM of the Jacobian (the left Jacobian of SO(3),
its series below |w| = 1e-2, the association of csrc/geom.hpp corner_jacobian).  Nothing of that is here.  This module states the FORWARD
model only -- Rodrigues matrix, pc = R_c^T (R_f (R_m X + t_m) + t_f - t_c), the pinhole division, the residual observed - projected in both
residual modes, the Huber weight -- for real and for complex arrays, and differentiates it by the complex step

    d r / d x_k = Im r(x + i h e_k) / h,   h = 1e-30,

which has no subtraction of nearby values and hence no step-size trade-off: the derivative is as good as the forward evaluation.

Every observation depends on 18 pose parameters (camera, marker, frame) and, with the intrinsics block, on (fx, cx, fy, cy) of its camera.
"Parameter k of every observation's camera / marker / frame" is perturbed for all observations at once: 18 (+ 4) evaluations give all
8 x 18 (8 x 22) blocks at any N.  No dense 8N x P Jacobian is ever built; the normal equations are assembled from the per-observation Gram
matrices, slice by slice.

With Huber the reference follows the product's contract (csrc/geom.hpp corner_residual): the residual rows are weighted, the Jacobian is not.
"""
import numpy as np

CSTEP = 1e-30
SERIES_BELOW = 1e-3          # |theta| below which sin(t)/t and 2 sin^2(t/2)/t^2 are taken from their series through t^6
RES_F32, RES_F64 = 0, 1      # as aar.RES_F32 / aar.RES_F64
# scaled_error() of the oracle's analytic H against this reference, the largest over every golden fixture and every edge data set on the
# CPU (tests/test_projection_reference_host.py, where it is measured and printed), and the bar for oracle and device alike: 100 x that.
# The factor covers the different summation orders of atomics, wave sums and chunk partials over up to ~1e3 terms per entry.
SCALED_MEASURED = 5.0e-14
SCALED_BAR = 100 * SCALED_MEASURED


# ---------------------------------------------------------------- forward model (real or complex)
def rodrigues(w):
    """R = I + a [w]x + b [w]x^2 for w[..., 3], real or complex.  theta = sqrt(w . w) WITHOUT conjugate, so R is analytic in w."""
    w = np.asarray(w)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    t2 = x * x + y * y + z * z
    small = np.abs(t2) < SERIES_BELOW * SERIES_BELOW
    ser_a = 1 - t2 / 6 + t2 * t2 / 120 - t2 * t2 * t2 / 5040
    ser_b = 0.5 - t2 / 24 + t2 * t2 / 720 - t2 * t2 * t2 / 40320
    th = np.sqrt(np.where(small, 1, t2))        # (the series see t2 only: exactly zero works)
    sh = np.sin(th / 2)
    a = np.where(small, ser_a, np.sin(th) / th)
    b = np.where(small, ser_b, 2 * sh * sh / (th * th))
    R = np.empty(w.shape[:-1] + (3, 3), dtype=w.dtype if np.iscomplexobj(w) else np.float64)
    R[..., 0, 0] = 1 - b * (y * y + z * z); R[..., 0, 1] = -a * z + b * x * y;      R[..., 0, 2] = a * y + b * x * z
    R[..., 1, 0] = a * z + b * x * y;       R[..., 1, 1] = 1 - b * (x * x + z * z); R[..., 1, 2] = -a * x + b * y * z
    R[..., 2, 0] = -a * y + b * x * z;      R[..., 2, 1] = a * x + b * y * z;       R[..., 2, 2] = 1 - b * (x * x + y * y)
    return R


def half_size(marker_size):
    """half the marker's side as the product and the oracle take it: the division in float"""
    return float(np.float32(marker_size) / np.float32(2))


def corners(h):
    return np.array([[-h, h, 0.0], [h, h, 0.0], [h, -h, 0.0], [-h, -h, 0.0]])


def camera_points(pc6, pm6, pf6, h):
    """[N, 4, 3] corner positions in the camera's frame; p*6[N, 6] = (rotation vector, translation) of each observation's entities"""
    Rc, Rm, Rf = rodrigues(pc6[:, :3]), rodrigues(pm6[:, :3]), rodrigues(pf6[:, :3])
    X = corners(h)
    q = np.einsum("nij,kj->nki", Rm, X) + pm6[:, None, 3:]
    s = np.einsum("nij,nkj->nki", Rf, q) + pf6[:, None, 3:]
    return np.einsum("nji,nkj->nki", Rc, s - pc6[:, None, 3:])


def project(pc6, pm6, pf6, K, h):
    """[N, 8] pixel coordinates (u0 v0 .. u3 v3); K[N, 3, 3]"""
    p = camera_points(pc6, pm6, pf6, h)
    hh = np.einsum("nij,nkj->nki", K, p)
    uv = hh[..., :2] / hh[..., 2:3]
    return uv.reshape(len(p), 8)


def huber_weight(e, delta):
    """sqrt(rho(e) / e), rho(e) = e up to delta^2 and 2 delta sqrt(e) - delta^2 beyond, delta^2 and 2 delta rounded to float; 1 at e = 0"""
    d = np.float32(delta)
    dsq, d2 = float(d * d), float(np.float32(2) * d)
    es = np.where(e == 0, 1.0, e)
    rho = np.where(es <= dsq, es, d2 * np.sqrt(es) - dsq)
    return np.where(e == 0, 1.0, np.sqrt(rho / es))


def residual_rows(uv_obs, uv_proj, res_mode, huber_delta=None):
    """[N, 8] rows observed - projected.  RES_F32: the projection is stored as float and subtracted in float (the float-faithful mode)."""
    obs = np.asarray(uv_obs, dtype=np.float32).reshape(-1, 8)
    if res_mode == RES_F32:
        r = (obs - uv_proj.astype(np.float32)).astype(np.float64)
    else:
        r = obs.astype(np.float64) - uv_proj
    if huber_delta is not None:
        rr = r.reshape(-1, 4, 2)
        w = huber_weight(rr[..., 0] ** 2 + rr[..., 1] ** 2, huber_delta)
        r = (rr * w[..., None]).reshape(-1, 8)
    return r


# ---------------------------------------------------------------- a problem: which parameters, where in z
class Reference:
    """The reference bound to a data set (an aar.Dataset-like object) with the switches of a Problem.

    z order as Problem / the oracle's Layout: cameras without the root (6 each), markers without the root, frames, then -- with
    intrinsics -- 9 per camera, the root included: fx, cx, fy, cy and five entries nothing depends on (their rows and columns of H are zero,
    as the device reports them).  A switched-off group has no columns.  With intrinsics the camera matrix is [fx 0 cx; 0 fy cy; 0 0 1]
    (a skew in the data set's matrix is dropped, as in the product); without, the data set's matrix as it stands."""

    def __init__(self, ds, optimize=(True, True, True), intrinsics=False, huber_delta=None):
        self.ds = ds
        self.C, self.M, self.F = int(ds.num_cams), int(ds.num_markers), int(ds.num_frames)
        self.rc, self.rm = int(ds.root_cam), int(ds.root_marker)
        self.oc, self.om, self.of = [bool(b) for b in optimize]
        self.intr = bool(intrinsics)
        self.huber_delta = huber_delta
        self.h = half_size(ds.marker_size)
        self.oc_ = np.asarray(ds.obs_cam, dtype=np.int64)
        self.om_ = np.asarray(ds.obs_marker, dtype=np.int64)
        self.of_ = np.asarray(ds.obs_frame, dtype=np.int64)
        self.uv = np.asarray(ds.obs_uv, dtype=np.float32).reshape(-1, 8)
        self.N = len(self.oc_)
        C, M, F = self.C, self.M, self.F
        o = 0
        self.z_cam0 = self.z_mk0 = self.z_fr0 = self.z_intr0 = -1
        if self.oc:
            self.z_cam0 = o; o += 6 * (C - 1)
        if self.om:
            self.z_mk0 = o; o += 6 * (M - 1)
        if self.of:
            self.z_fr0 = o; o += 6 * F
        if self.intr:
            self.z_intr0 = o; o += 9 * C
        self.P = o
        self.npar = 22 if self.intr else 18

    # -- per-entity 6-vectors from x_full (roots: zeros, i.e. the identity)
    def entity_vectors(self, x_full):
        x = np.asarray(x_full, dtype=np.float64)
        C, M, F = self.C, self.M, self.F
        cam = np.zeros((C, 6)); mk = np.zeros((M, 6))
        cam[np.arange(C) != self.rc] = x[:6 * (C - 1)].reshape(C - 1, 6)
        mk[np.arange(M) != self.rm] = x[6 * (C - 1):6 * (C - 1) + 6 * (M - 1)].reshape(M - 1, 6)
        n0 = 6 * (C - 1) + 6 * (M - 1)
        fr = x[n0:n0 + 6 * F].reshape(F, 6)
        return cam, mk, fr

    def camera_matrices(self, x_full):
        """(K[C, 3, 3], q): the camera matrices in force at x_full.  Without the intrinsics block the data set's matrices and q = None; with
        it q[C, 4] = (fx, cx, fy, cy) from the 9 per camera at the end of x_full (the data set's own where x_full carries none) and
        K = [fx 0 cx; 0 fy cy; 0 0 1] built from q"""
        K = np.asarray(self.ds.cam_mats, dtype=np.float64).reshape(self.C, 3, 3).copy()
        if not self.intr:
            return K, None
        x = np.asarray(x_full, dtype=np.float64)
        n0 = 6 * (self.C - 1) + 6 * (self.M - 1) + 6 * self.F
        q = x[n0:n0 + 9 * self.C].reshape(self.C, 9)[:, :4].copy() if len(x) > n0 else np.stack([K[:, 0, 0], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2]], axis=1)
        return self._K_from_intr(q), q

    @staticmethod
    def _K_from_intr(q):
        K = np.zeros((len(q), 3, 3), dtype=q.dtype)
        K[:, 0, 0] = q[:, 0]; K[:, 0, 2] = q[:, 1]; K[:, 1, 1] = q[:, 2]; K[:, 1, 2] = q[:, 3]; K[:, 2, 2] = 1
        return K

    def _obs_params(self, x_full, sl):
        cam, mk, fr = self.entity_vectors(x_full)
        K, q = self.camera_matrices(x_full)
        c, m, f = self.oc_[sl], self.om_[sl], self.of_[sl]
        return cam[c], mk[m], fr[f], K[c], (q[c] if q is not None else None)

    def columns(self, sl=slice(None)):
        """[n, npar] column of z each of an observation's parameters lands in, -1 where it has none (root, switched-off group)"""
        c, m, f = self.oc_[sl], self.om_[sl], self.of_[sl]
        n = len(c)
        col = np.full((n, self.npar), -1, dtype=np.int64)
        k6 = np.arange(6)
        if self.oc:
            slot = np.where(c < self.rc, c, c - 1)
            col[:, 0:6] = np.where((c != self.rc)[:, None], self.z_cam0 + 6 * slot[:, None] + k6, -1)
        if self.om:
            slot = np.where(m < self.rm, m, m - 1)
            col[:, 6:12] = np.where((m != self.rm)[:, None], self.z_mk0 + 6 * slot[:, None] + k6, -1)
        if self.of:
            col[:, 12:18] = self.z_fr0 + 6 * f[:, None] + k6
        if self.intr:
            col[:, 18:22] = self.z_intr0 + 9 * c[:, None] + np.arange(4)
        return col

    def projection(self, x_full, sl=slice(None)):
        pc, pm, pf, K, q = self._obs_params(x_full, sl)
        return project(pc, pm, pf, K, self.h)

    def residuals(self, x_full, res_mode=RES_F64, sl=slice(None)):
        """[8 n] residual rows of the observations in sl, in the data set's order"""
        return residual_rows(self.uv[sl], self.projection(x_full, sl), res_mode, self.huber_delta).reshape(-1)

    def blocks(self, x_full, sl=slice(None)):
        """G[n, 8, npar] = d(projection) / d(parameter) by the complex step (d r / d parameter = -G): columns 0-5 the camera's 6-vector,
        6-11 the marker's, 12-17 the frame's, 18-21 (fx, cx, fy, cy)"""
        pc, pm, pf, K, q = self._obs_params(x_full, sl)
        n = len(pc)
        G = np.empty((n, 8, self.npar))
        base = [pc.astype(np.complex128), pm.astype(np.complex128), pf.astype(np.complex128)]
        Kc = K.astype(np.complex128)
        G[...] = 0
        for g in range(3):
            if not (self.oc, self.om, self.of)[g]:
                continue                                   # a switched-off group has no columns: its evaluations are not needed
            for k in range(6):
                args = list(base)
                a = base[g].copy()
                a[:, k] += 1j * CSTEP
                args[g] = a
                G[:, :, 6 * g + k] = project(args[0], args[1], args[2], Kc, self.h).imag / CSTEP
        if self.intr:
            for k in range(4):
                qq = q.astype(np.complex128)
                qq[:, k] += 1j * CSTEP
                G[:, :, 18 + k] = project(base[0], base[1], base[2], self._K_from_intr(qq), self.h).imag / CSTEP
        return G

    def jacobian_blocks(self, x_full, sl=slice(None)):
        """(J[n, 8, npar], col[n, npar]): the Jacobian of the residual rows, -G, with the z column of each entry"""
        return -self.blocks(x_full, sl), self.columns(sl)

    def normal_equations(self, x_full, res_mode=RES_F64, slice_len=16384):
        """dense (H, B, ss) = (J^T J, -J^T r, r^T r) in z order, streamed over slices of observations; slice partials are added in long double"""
        P = self.P
        acc = np.longdouble if self.N > slice_len else np.float64     # (one slice: nothing to add up across slices)
        Hacc = np.zeros((P + 1) * (P + 1), dtype=acc)
        Bacc = np.zeros(P + 1, dtype=acc)
        ss = np.longdouble(0)
        for s0 in range(0, self.N, slice_len):
            sl = slice(s0, min(self.N, s0 + slice_len))
            G = self.blocks(x_full, sl)
            r = self.residuals(x_full, res_mode, sl).reshape(-1, 8)
            col = self.columns(sl)
            col = np.where(col < 0, P, col)
            GG = np.einsum("nra,nrb->nab", G, G)
            Gr = np.einsum("nra,nr->na", G, r)
            idx = (col[:, :, None] * (P + 1) + col[:, None, :]).reshape(-1)
            Hacc += np.bincount(idx, weights=GG.reshape(-1), minlength=(P + 1) * (P + 1))
            Bacc += np.bincount(col.reshape(-1), weights=Gr.reshape(-1), minlength=P + 1)
            ss += np.longdouble((r.astype(np.longdouble) ** 2).sum())
        H = Hacc.reshape(P + 1, P + 1)[:P, :P].astype(np.float64)
        return H, Bacc[:P].astype(np.float64), float(ss)


def scaled_error(H, Href):
    """max |H - Href|_ij / sqrt(H_ii H_jj) over the non-zero diagonal of Href: the measure that max|H| hides the small blocks from"""
    d = np.sqrt(np.abs(np.diag(Href)))
    nz = d > 0
    s = np.outer(d[nz], d[nz])
    return float((np.abs(H - Href)[np.ix_(nz, nz)] / s).max())


# ---------------------------------------------------------------- data sets at given poses
def rotvec(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    return a / np.linalg.norm(a) * angle


def build_dataset(cams6, markers6, frames6, obs_frame, obs_cam, obs_marker, K=None, marker_size=0.1, noise_px=0.5, seed=1,
                  root_cam=0, root_marker=0, dataset_cls=None):
    """An aar.Dataset (or any class given) filled field by field: cameras [C, 6], markers [M, 6], frames [F, 6] AT THE GIVEN 6-vectors (the
    root entries are ignored: roots are the identity), the given observation triplets (ordered by frame), corners projected by this
    reference at those poses plus Gaussian noise, rounded to float.  Every corner must have positive depth of at least 5 % of its distance
    to the camera; a triplet that does not is an error."""
    if dataset_cls is None:
        import aar
        dataset_cls = aar.Dataset
    cams6 = np.array(cams6, dtype=np.float64).reshape(-1, 6); markers6 = np.array(markers6, dtype=np.float64).reshape(-1, 6)
    frames6 = np.array(frames6, dtype=np.float64).reshape(-1, 6)
    cams6[root_cam] = 0; markers6[root_marker] = 0
    C, M, F = len(cams6), len(markers6), len(frames6)
    of = np.asarray(obs_frame, dtype=np.int32); oc = np.asarray(obs_cam, dtype=np.int32); om = np.asarray(obs_marker, dtype=np.int32)
    if len(of) and (np.diff(of) < 0).any():
        raise ValueError("observations must be ordered by frame")
    for a, n in ((of, F), (oc, C), (om, M)):
        if len(a) and (a.min() < 0 or a.max() >= n):
            raise ValueError("observation index out of range")
    if K is None:
        K = np.array([[900.0, 0, 640.0], [0, 910.0, 360.0], [0, 0, 1]])
    K = np.broadcast_to(np.asarray(K, dtype=np.float64).reshape(-1, 3, 3), (C, 3, 3)).copy()
    ds = dataset_cls()
    ds.num_cams, ds.num_markers, ds.num_frames, ds.root_cam, ds.root_marker = C, M, F, int(root_cam), int(root_marker)
    ds.marker_size = float(marker_size)
    ds.cam_ids = np.arange(C, dtype=np.int32); ds.marker_ids = np.arange(M, dtype=np.int32); ds.frame_ids = np.arange(F, dtype=np.int32)
    ds.image_sizes = np.tile(np.array([1280, 720], dtype=np.int32), (C, 1))
    ds.cam_mats = K.reshape(C, 9)
    ds.dist_coeffs = np.zeros((C, 5))
    ds.obs_frame, ds.obs_cam, ds.obs_marker = of, oc, om
    ds.num_obs = len(of)
    keep_c = np.arange(C) != root_cam; keep_m = np.arange(M) != root_marker
    ds.x_full = np.concatenate([cams6[keep_c].reshape(-1), markers6[keep_m].reshape(-1), frames6.reshape(-1)])
    ds.x_truth = ds.x_full.copy()
    ds.optimize_cam_poses = ds.optimize_marker_poses = ds.optimize_object_poses = True
    ds.optimize_cam_intrinsics = False
    h = half_size(marker_size)
    p = camera_points(cams6[oc], markers6[om], frames6[of], h)
    depth, dist = p[..., 2], np.linalg.norm(p, axis=-1)
    bad = ~((depth > 0) & (depth >= 0.05 * dist))
    if bad.any():
        o = int(np.argwhere(bad)[0, 0])
        raise ValueError("observation %d (frame %d, camera %d, marker %d) sits at the projective pole: depth %.3g of distance %.3g"
                         % (o, of[o], oc[o], om[o], depth[o].min(), dist[o].max()))
    uv = project(cams6[oc], markers6[om], frames6[of], K[oc], h)
    rng = np.random.default_rng(seed)
    ds.obs_uv = (uv + noise_px * rng.standard_normal(uv.shape)).astype(np.float32)
    return ds


def visible_triplets(cams6, markers6, frames6, marker_size=0.1, min_cos=0.3, root_cam=0, root_marker=0):
    """(obs_frame, obs_cam, obs_marker), ordered by frame then camera then marker, of every triplet whose four corners are in front of
    the camera with depth >= min_cos of their distance.  A helper to choose triplets the way a detector would; build_dataset then
    asserts each of them."""
    cams6 = np.array(cams6, dtype=np.float64).reshape(-1, 6); markers6 = np.array(markers6, dtype=np.float64).reshape(-1, 6)
    frames6 = np.array(frames6, dtype=np.float64).reshape(-1, 6)
    cams6[root_cam] = 0; markers6[root_marker] = 0
    C, M, F = len(cams6), len(markers6), len(frames6)
    f, c, m = [a.reshape(-1) for a in np.meshgrid(np.arange(F), np.arange(C), np.arange(M), indexing="ij")]
    p = camera_points(cams6[c], markers6[m], frames6[f], half_size(marker_size))
    ok = (p[..., 2] >= min_cos * np.linalg.norm(p, axis=-1)).all(axis=1)
    return f[ok].astype(np.int32), c[ok].astype(np.int32), m[ok].astype(np.int32)


# ---------------------------------------------------------------- the edge-pose data sets (host and GPU tests share them)
EDGE_ANGLES = [0.0, 1e-20, 1e-17, 3e-16, 1e-9, 1e-5, 0.01 - 1e-6, 0.01 + 1e-6, np.pi - 1e-9, np.pi, np.pi + 1e-9, 2 * np.pi - 1e-3]
OBJECT_CENTRE = np.array([0.0, 0.0, 3.0])


def camera_looking_at_centre(w, jitter=0.0):
    """the 6-vector of a camera with rotation vector w that has OBJECT_CENTRE three units down its optical axis (plus jitter)"""
    R = rodrigues(np.asarray(w, dtype=np.float64))
    return np.concatenate([w, OBJECT_CENTRE - R @ np.array([0.0, 0.0, 3.0]) + jitter])


def edge_dataset(theta, board=False, zero_translation=False, seed=7, C=5, M=7, F=9, noise_px=0.7, eval_shift=2e-3):
    """A small data set with sensible geometry -- cameras three units from a board-sized object, every corner well in front of its
    camera -- in which camera 1, marker 1 and frame 1 carry a rotation of exactly `theta` about random axes (board=True: ALL markers,
    the coplanar-board case), and with zero_translation those three entities sit at translation zero as well.  Cameras 2 and 3 are
    turned far round (2.0 and 2.5 rad) so that an object at the origin is still in front of somebody.  The triplets are those a detector
    would see (visible_triplets).  ds.x_full is the evaluation point: the truth with the translations of the other entities shifted by
    ~eval_shift, so residuals are a few pixels, while every edge rotation (and zero translation) is exactly as given."""
    rng = np.random.default_rng(seed)

    def axis():
        a = rng.standard_normal(3)
        return a / np.linalg.norm(a)

    cams = np.zeros((C, 6)); mks = np.zeros((M, 6)); frs = np.zeros((F, 6))
    for c in range(1, C):
        ang = {2: 2.0, 3: 2.5}.get(c, rng.uniform(0.15, 0.5))
        w = rotvec(axis() * [1, 1, 0.3], ang)
        cams[c] = camera_looking_at_centre(w, 0.1 * rng.standard_normal(3))
    for m in range(1, M):
        mks[m, :3] = rotvec(axis(), rng.uniform(0.1, 0.6))
        mks[m, 3:] = [0.16 * ((m % 3) - 1), 0.16 * ((m // 3) - 1), 0.02 * rng.standard_normal()]
    for f in range(F):
        frs[f, :3] = rotvec(axis(), rng.uniform(0.2, 0.7))
        frs[f, 3:] = OBJECT_CENTRE + 0.15 * rng.standard_normal(3)
    edge_c, edge_m, edge_f = [1], (list(range(1, M)) if board else [1]), [1]
    for c in edge_c:
        cams[c] = camera_looking_at_centre(rotvec(axis(), theta), 0.1 * rng.standard_normal(3))
    for m in edge_m:
        mks[m, :3] = rotvec(axis(), theta)
    for f in edge_f:
        frs[f, :3] = rotvec(axis(), theta)
    if zero_translation:
        cams[1, 3:] = 0; mks[1, 3:] = 0; frs[1, 3:] = 0
    of, oc, om = visible_triplets(cams, mks, frs)
    for name, arr, idx in (("camera", oc, 1), ("marker", om, 1), ("frame", of, 1)):
        if (arr == idx).sum() < 2:
            raise ValueError("edge %s %d has fewer than two observations at theta = %r" % (name, idx, theta))
    ds = build_dataset(cams, mks, frs, of, oc, om, noise_px=noise_px, seed=seed + 1)
    shift = eval_shift * rng.standard_normal((C - 1 + M - 1 + F, 3))
    x = ds.x_full.reshape(-1, 6).copy()
    fixed = np.zeros(len(x), dtype=bool)
    if zero_translation:
        fixed[[0, (C - 1) + 0, (C - 1) + (M - 1) + 1]] = True     # camera 1, marker 1, frame 1 in x_full's root-skipping order
    x[~fixed, 3:] += shift[~fixed]
    ds.x_full = x.reshape(-1)
    # corner 0 of observation 0 is observed exactly where the float-faithful mode projects it: e = 0, the branch of the Huber weight that divides by nothing
    ds.obs_uv = np.array(ds.obs_uv, dtype=np.float32).reshape(-1, 8)
    ds.obs_uv[0, 0:2] = Reference(ds).projection(ds.x_full, slice(0, 1))[0, 0:2].astype(np.float32)
    return ds


def other_chart(x_full, entity_rows):
    """x_full with the rotation vectors of the given rows (of its [.., 6] view) moved to theta + 2 pi: the same rotations, another chart"""
    x = np.array(x_full, dtype=np.float64).reshape(-1, 6).copy()
    for i in entity_rows:
        th = np.linalg.norm(x[i, :3])
        x[i, :3] *= (th + 2 * np.pi) / th
    return x.reshape(-1)


# ---------------------------------------------------------------- data sets with prescribed shapes (pass A workgroups, pass B chunks)
def rig(C, M, F, seed, grid=None):
    """cameras on an arc three units from the object centre, all looking at it (camera 0, the root, at the origin), M markers on a
    board-like grid with small tilts, F object poses near the centre with moderate rotations: every marker is in front of every camera"""
    rng = np.random.default_rng(seed)

    def axis(scale=(1, 1, 1)):
        a = rng.standard_normal(3) * scale
        return a / np.linalg.norm(a)

    cams = np.zeros((C, 6)); mks = np.zeros((M, 6)); frs = np.zeros((F, 6))
    for c in range(1, C):
        cams[c] = camera_looking_at_centre(rotvec(axis((0.4, 1, 0.2)), rng.uniform(0.15, 0.8)), 0.1 * rng.standard_normal(3))
    cols = grid or int(np.ceil(np.sqrt(M)))
    for m in range(1, M):
        mks[m, :3] = rotvec(axis(), rng.uniform(0.05, 0.3))
        mks[m, 3:] = [0.13 * (m % cols), 0.13 * (m // cols), 0.01 * rng.standard_normal()]
    mks[1:, 3:5] -= mks[:, 3:5].mean(axis=0)
    frs[:, :3] = [rotvec(axis(), rng.uniform(0.05, 0.4)) for _ in range(F)]
    frs[:, 3:] = OBJECT_CENTRE + 0.1 * rng.standard_normal((F, 3))
    return cams, mks, frs


def _shift_evaluation_point(ds, seed, rot=1e-3, trans=2e-3):
    rng = np.random.default_rng(seed)
    x = ds.x_full.reshape(-1, 6).copy()
    x[:, :3] += rot * rng.standard_normal((len(x), 3))
    x[:, 3:] += trans * rng.standard_normal((len(x), 3))
    ds.x_full = x.reshape(-1)
    return ds


def frame_counts_dataset(counts, C=8, M=40, seed=11):
    """frame f carries exactly counts[f] observations: the first counts[f] of the C x M (camera, marker) pairs in a shuffled order of its
    own, stored camera-major -- so a frame with one observation touches 2 entities and one with C x M of them touches every camera and marker"""
    counts = [int(n) for n in counts]
    if max(counts) > C * M:
        raise ValueError("a frame cannot carry %d observations of %d x %d pairs" % (max(counts), C, M))
    cams, mks, frs = rig(C, M, len(counts), seed)
    rng = np.random.default_rng(seed + 1)
    of, oc, om = [], [], []
    for f, n in enumerate(counts):
        pick = np.sort(rng.permutation(C * M)[:n])
        of += [f] * n; oc += list(pick // M); om += list(pick % M)
    ds = build_dataset(cams, mks, frs, of, oc, om, noise_px=0.7, seed=seed + 2)
    return _shift_evaluation_point(ds, seed + 3)


def run_lengths_dataset(lengths, C=3, M=6, seed=13, F=None):
    """(camera, marker) run i has exactly lengths[i] observations, one in each of the frames 0 .. lengths[i] - 1; run i is pair number i of
    the C x M pairs in a shuffled order (root camera and root marker among them)"""
    lengths = [int(n) for n in lengths]
    if len(lengths) > C * M:
        raise ValueError("%d runs need more than %d x %d pairs" % (len(lengths), C, M))
    F = max(lengths) if F is None else F
    if F < max(lengths):
        raise ValueError("a run of %d needs that many frames" % max(lengths))
    cams, mks, frs = rig(C, M, F, seed)
    pairs = np.random.default_rng(seed + 1).permutation(C * M)[:len(lengths)]
    of, oc, om = [], [], []
    for f in range(F):
        here = np.sort([p for p, n in zip(pairs, lengths) if n > f])
        of += [f] * len(here); oc += [int(p) // M for p in here]; om += [int(p) % M for p in here]
    ds = build_dataset(cams, mks, frs, of, oc, om, noise_px=0.7, seed=seed + 2)
    return _shift_evaluation_point(ds, seed + 3)


def cut_frames(ds, n_frames, dataset_cls=None):
    """the first n_frames frames of a data set, its arrays cut in numpy"""
    import copy
    sub = copy.copy(ds)
    keep = np.asarray(ds.obs_frame) < n_frames
    for k in ("obs_frame", "obs_cam", "obs_marker", "obs_uv"):
        setattr(sub, k, np.ascontiguousarray(np.asarray(getattr(ds, k))[keep]))
    sub.num_obs = int(keep.sum())
    sub.num_frames = n_frames
    sub.frame_ids = np.asarray(ds.frame_ids)[:n_frames].copy()
    n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    sub.x_full = np.asarray(ds.x_full)[:n0 + 6 * n_frames].copy()
    sub.x_truth = None
    return sub
