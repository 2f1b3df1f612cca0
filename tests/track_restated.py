"""float64 restatement of MultiCamMapper::track() for one frame -- TEST INFRASTRUCTURE ONLY.

What k_track (automatic-ar_amd/csrc/eval_kernels.hip) runs on the device for every frame, written again in numpy and independent of
both csrc/geom.hpp and oracle/ba_oracle.cpp:

    projection   p = R_c^T (R_f (R_m X + t_m) + t_f - t_c),  (u, v) = (K p)_xy / (K p)_z,  X = corner k of the marker model
                 (-h, h, 0) (h, h, 0) (h, -h, 0) (-h, -h, 0), h = float(marker_size) / 2 rounded to float
    residual     (double)ou - u per corner, kept in double (error_function_tracking)
    Huber        r_w = w r,  w = sqrt(rho / e),  e = |r|^2,  rho = 2 delta sqrt(e) - delta^2 with delta^2 and 2 delta rounded to
                 float32; e == 0 and e <= delta^2 leave w = 1.  delta < 0: no weights.
    Jacobian     complex step on the weighted residual, J[:, k] = Im r_w(z + i h e_k) / h, h = 1e-30: the derivative to rounding,
                 the weight's own derivative included, without an analytic derivation.  Branches are decided on the real part.
    LM           SparseLevMarq::solve / step as k_track restates them: mu = tau max diag(J^T J) on first use; a try solves
                 (J^T J + mu I) d = B = -J^T r_w, gain = (err - prevErr) / (0.5 (mu |d|^2 - d.B)); accepted when gain > 0 and
                 err < prevErr (then mu *= max(0.33, 1 - (2 gain - 1)^3), v = 2), otherwise mu *= v, v *= 5; at most 5 retries;
                 exit 1 (err < min_error), 2 (|prevErr - err| <= min_step, |prevErr - err| / rows <= min_avg or no accepted try),
                 3 (err > prevErr), rows = 8 x detections.

track_frame() also reports how close the decisions it took came to going the other way (`margin`): for each comparison
a <= b taken on errors, |a - b| relative to the error scale of the frame.  Two float64 runs whose errors agree to ~1e-12 take the
same branch wherever the margin is well above that.  An accept decision is left out where either outcome ends the loop in the same
iteration (the try lands within rows min_avg / 2 of prevErr): it decides the last rounding-level step, not the iteration count.
"""
import numpy as np

H_CS = 1e-30
MARGIN = 1e-9      # decisions closer than this (relative) may go either way between two float64 runs
CORNER_SX = np.array([-1.0, 1.0, 1.0, -1.0])
CORNER_SY = np.array([1.0, 1.0, -1.0, -1.0])


def hat(w):
    """[w]x for w [..., 3] (real or complex)"""
    z = np.zeros_like(w[..., 0])
    return np.stack([np.stack([z, -w[..., 2], w[..., 1]], -1),
                     np.stack([w[..., 2], z, -w[..., 0]], -1),
                     np.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def rodrigues(w):
    """rotation matrices of rotation vectors w [..., 3], real or complex (analytic in w: no conjugates, no abs).
    R = I + a [w]x + b [w]x^2 with a = sin(th)/th, b = (1 - cos th)/th^2, th^2 = w.w; Taylor series in th^2 near 0 (th = 0 exactly
    included, where the complex step still needs the first-order term)."""
    w = np.asarray(w)
    t2 = np.sum(w * w, axis=-1)
    small = np.abs(t2.real) < 1e-6
    th = np.sqrt(np.where(small, 1.0, t2))
    a = np.where(small, 1 - t2 / 6 + t2 * t2 / 120 - t2 ** 3 / 5040, np.sin(th) / th)
    b = np.where(small, 0.5 - t2 / 24 + t2 * t2 / 720 - t2 ** 3 / 40320, (1 - np.cos(th)) / np.where(small, 1.0, t2))
    W = hat(w)
    return np.eye(3) + a[..., None, None] * W + b[..., None, None] * (W @ W)


class TrackData:
    """The fixed part of a track() problem: camera and marker transforms, camera matrices and the detections, grouped by frame.

    ds: an aar.Dataset-like object; x_full: the pose vector (cameras / markers after the root-skipping layout, then the frames;
    with intrinsics=True followed by (fx cx fy cy d0..d4) per camera, from which K is rebuilt as [fx 0 cx; 0 fy cy; 0 0 1])."""

    def __init__(self, ds, x_full, intrinsics=False):
        x = np.asarray(x_full, dtype=np.float64)
        C, M, F = ds.num_cams, ds.num_markers, ds.num_frames
        self.C, self.M, self.F = C, M, F
        self.fr0 = 6 * (C - 1) + 6 * (M - 1)

        def poses(off, n, root):
            R = np.tile(np.eye(3), (n, 1, 1))
            t = np.zeros((n, 3))
            for i in range(n):
                if i == root:
                    continue
                v = x[off + 6 * (i if i < root else i - 1): off + 6 * (i if i < root else i - 1) + 6]
                R[i] = rodrigues(v[:3])
                t[i] = v[3:]
            return R, t

        self.Rc, self.tc = poses(0, C, ds.root_cam)
        self.Rm, self.tm = poses(6 * (C - 1), M, ds.root_marker)
        if intrinsics:
            q = x[self.fr0 + 6 * F:].reshape(C, 9)
            K = np.zeros((C, 3, 3))
            K[:, 0, 0], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2], K[:, 2, 2] = q[:, 0], q[:, 1], q[:, 2], q[:, 3], 1.0
        else:
            K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(C, 3, 3)
        self.K = K
        h = float(np.float32(np.float32(ds.marker_size) / np.float32(2)))
        self.X = np.stack([CORNER_SX * h, CORNER_SY * h, np.zeros(4)], -1)      # [4, 3]
        of = np.asarray(ds.obs_frame)
        order = np.argsort(of, kind="stable")
        self.start = np.searchsorted(of[order], np.arange(F + 1))
        self.cam = np.asarray(ds.obs_cam)[order]
        self.mk = np.asarray(ds.obs_marker)[order]
        self.uv = np.asarray(ds.obs_uv, dtype=np.float32).reshape(-1, 8)[order]
        self.z0 = x[self.fr0: self.fr0 + 6 * F].reshape(F, 6).copy()

    def frame(self, f):
        """what one frame's loop reads: (R_c^T, t_c, R_m X + t_m [n, 4, 3], K [n, 3, 3], observations [n, 4, 2] as double)"""
        s = slice(self.start[f], self.start[f + 1])
        c, m = self.cam[s], self.mk[s]
        q = np.einsum("nij,kj->nki", self.Rm[m], self.X) + self.tm[m][:, None, :]
        return dict(RcT=np.transpose(self.Rc[c], (0, 2, 1)), tc=self.tc[c], q=q, K=self.K[c],
                    ou=self.uv[s].astype(np.float64).reshape(-1, 4, 2))


def residuals(fd, zf):
    """unweighted residuals [..., n, 4, 2] of a frame at pose(s) zf [..., 6] (real or complex)"""
    zf = np.asarray(zf)
    Rf = rodrigues(zf[..., :3])                                                 # [..., 3, 3]
    s = np.einsum("...ij,nkj->...nki", Rf, fd["q"]) + zf[..., None, None, 3:]   # [..., n, 4, 3]
    y = s - fd["tc"][:, None, :]
    p = np.einsum("nij,...nkj->...nki", fd["RcT"], y)
    hp = np.einsum("nij,...nkj->...nki", fd["K"], p)
    uv = hp[..., :2] / hp[..., 2:3]
    return fd["ou"] - uv


def huber_weights(r, delta):
    """per-corner weights w [..., n, 4] as k_track applies them (see the module docstring); the branch on the real part of e"""
    e = r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]
    if delta is None or delta < 0:
        return np.ones_like(e), np.zeros(e.shape, dtype=bool)
    dsq = float(np.float32(delta) * np.float32(delta))
    d2 = float(np.float32(2) * np.float32(delta))
    out = (e.real != 0.0) & (e.real > dsq)
    es = np.where(out, e, 1.0)
    rho = np.where(out, d2 * np.sqrt(es) - dsq, es)
    return np.where(out, np.sqrt(rho / es), 1.0), out


def weighted(fd, zf, delta):
    r = residuals(fd, zf)
    w, out = huber_weights(r, delta)
    return r * w[..., None], out


def frame_error(fd, zf, delta):
    rw, _ = weighted(fd, zf, delta)
    return float(np.sum(rw * rw))


def jacobian(fd, zf, delta, h=H_CS):
    """(J [8n, 6] = d r_w / d z by complex step, r_w [8n]) at the real pose zf"""
    zf = np.asarray(zf, dtype=np.float64)
    zc = zf[None, :] + 1j * h * np.eye(6)
    rc, _ = weighted(fd, zc, delta)                      # [6, n, 4, 2]
    J = (rc.imag / h).reshape(6, -1).T
    rw, _ = weighted(fd, zf, delta)
    return J, rw.reshape(-1)


def _margin(a, b, scale):
    if a == b:
        return np.inf if a == 0.0 or scale == 0.0 else 0.0
    return abs(a - b) / max(scale, abs(a), abs(b))


def track_frame(fd, z0, delta=-1.0, max_iters=10000, min_error=1e-5, min_step=0.0, min_avg=1e-4, tau=1.0):
    """k_track's loop for one frame (TrackData.frame(f)) from pose z0.  Returns a dict: z (pose), iterations, err, exit (0: cap or no
    detection), rejected (tries not accepted), last_accepted (the last iteration ended with an accepted try), outliers (corners past delta at the final pose), margin (see the module docstring), slack (the largest step |d|_inf whose accept decision was within MARGIN:
    a rounding-level step one run may take and the other not)."""
    z = np.array(z0, dtype=np.float64)
    n = fd["ou"].shape[0]
    rows = 8.0 * n
    curr = frame_error(fd, z, delta)
    prev = curr
    mu, v = -1.0, 2.0
    must, iters, rejected = 0, 0, 0
    margin = np.inf
    slack = 0.0        # largest step whose acceptance was within MARGIN: two runs may end up that far apart
    it, accepted = 0, False
    while it < max_iters and not must and rows > 0:
        J, rw = jacobian(fd, z, delta)
        V = J.T @ J
        B = -J.T @ rw
        if mu < 0:
            mu = float(np.max(np.diag(V))) * tau
        ntries, accepted = 0, False
        while True:
            d = np.linalg.solve(V + mu * np.eye(6), B)
            zt = z + d
            err = frame_error(fd, zt, delta)
            d2, dg = float(d @ d), float(d @ B)
            Lq = 0.5 * (mu * d2 - dg)
            with np.errstate(divide="ignore", invalid="ignore"):
                gain = float(np.float64(err - prev) / np.float64(Lq))   # 0/0 = NaN as on the device
            # an accept decision counts only where its outcome can change the iteration count: a try within rows min_avg / 2 of
            # prevErr ends the loop in this iteration either way (accepted: the average-step test; rejected: the retries find
            # nothing much better than a point that close to the optimum, and no accepted try exits too)
            if abs(err - prev) > 0.5 * rows * min_avg:
                margin = min(margin, _margin(err, prev, max(err, prev)), _margin(mu * d2, dg, abs(mu * d2) + abs(dg)))
            if _margin(err, prev, max(err, prev)) <= MARGIN:
                slack = max(slack, float(np.abs(d).max()))
            if gain > 0 and err - prev < 0:
                t = 2 * gain - 1
                mu = mu * max(0.33, 1.0 - t * t * t)
                v = 2.0
                curr = err
                z = zt
                accepted = True
            else:
                mu, v = mu * v, v * 5
                rejected += 1
            if not (gain <= 0):
                break
            ntries += 1
            if not (ntries - 1 < 5) or accepted:
                break
        scale = max(prev, curr)
        if curr < min_error:
            must = 1
        margin = min(margin, _margin(curr, min_error, max(curr, min_error)))
        dd = abs(prev - curr)
        if dd <= min_step or abs((prev - curr) / rows) <= min_avg or not accepted:
            must = 2
        # (with min_step = 0 that test is dd == 0, i.e. no accepted try: the accept decision's margin covers it)
        margin = min(margin, _margin(dd, min_step, max(scale, min_step)) if min_step > 0 else np.inf,
                     _margin(dd, rows * min_avg, max(scale, rows * min_avg)))
        if curr > prev:
            must = 3
        iters += 1
        prev = curr
        it += 1
    _, out = weighted(fd, z, delta)
    return dict(z=z, iterations=iters, err=curr, exit=must, rejected=rejected, last_accepted=bool(iters == 0 or accepted),
                outliers=int(out.sum()), margin=margin, slack=slack)


def track_all(ds, x_full, delta=-1.0, intrinsics=False, frames=None, **lm):
    """track_frame over every frame (or `frames`): (x_full with the refined frame poses, list of per-frame dicts)"""
    td = TrackData(ds, x_full, intrinsics=intrinsics)
    x = np.array(x_full, dtype=np.float64)
    res = []
    for f in (range(ds.num_frames) if frames is None else frames):
        r = track_frame(td.frame(f), td.z0[f], delta=delta, **lm)
        r["frame"] = f
        r["detections"] = int(td.start[f + 1] - td.start[f])
        x[td.fr0 + 6 * f: td.fr0 + 6 * f + 6] = r["z"]
        res.append(r)
    return x, res
