"""float64 restatement of smoothed tracking (aar_track_smooth) -- TEST INFRASTRUCTURE ONLY.

Built on tests/track_restated.py (TrackData, weighted, rodrigues: imported, not edited) and independent of csrc/smooth_kernels.hip:

    cost         E(z) = sum_f E_f(z_f) + sum_{f < F-1} e_f^T L_f e_f, E_f = track_restated.frame_error
    between      e_f = [ log((R_f dR_f)^T R_{f+1})^v ; t_{f+1} - t_f - dt_f ],  L_f = diag(1 / (sigma_rot^2 D_f) x3, 1 / (sigma_trans^2 D_f) x3),
                 D_f = frame_time[f+1] - frame_time[f] (1 without frame_time), (dR_f, dt_f) = rel_motion[f] as (rvec, t) or identity / zero
    Jacobian     complex step on e_f over the twelve entries of (z_f, z_{f+1}), h = 1e-30: no analytic derivation.  The rotation log is
                 written for that: phi = (theta / sin theta) vee(Q - Q^T) / 2 with theta / sin theta as a series in sin^2 near 0 and theta =
                 atan2(s, c) carried to first order in the imaginary parts elsewhere.  Valid for rotation angles of e_f below ~3.1 rad.
    system       H_ff = V_f + J_a^T L_f J_a + J_b'^T L_{f-1} J_b',  H_{f,f+1} = J_a^T L_f J_b,  b = -(J^T r_w + J_e^T L e)
    solve        scipy.linalg.solveh_banded (numpy.linalg.solve on the dense matrix without scipy)
    LM           track_restated.track_frame's loop and its margin / slack bookkeeping over all 6F unknowns, rows = 8 N + 6 (F - 1)
"""
import numpy as np

import track_restated as tr

try:
    from scipy.linalg import solveh_banded
except ImportError:   # pragma: no cover
    solveh_banded = None

H_CS = tr.H_CS
MARGIN = tr.MARGIN


def so3_log(Q):
    """log(Q)^v of rotation matrices Q [..., 3, 3], real or complex (a real rotation plus a first-order imaginary perturbation)"""
    Q = np.asarray(Q)
    v = np.stack([Q[..., 2, 1] - Q[..., 1, 2], Q[..., 0, 2] - Q[..., 2, 0], Q[..., 1, 0] - Q[..., 0, 1]], -1)   # 2 sin(theta) n
    c = 0.5 * (Q[..., 0, 0] + Q[..., 1, 1] + Q[..., 2, 2] - 1.0)
    s2 = np.sum(v * v, axis=-1) / 4                      # sin^2(theta), analytic in Q
    small = (np.abs(s2.real) < 1e-6) & (c.real > 0)
    # asin(s) / s = 1 + s^2/6 + 3 s^4/40 + 15 s^6/336 + 105 s^8/3456
    ser = 1 + s2 / 6 + 3 * s2 ** 2 / 40 + 15 * s2 ** 3 / 336 + 105 * s2 ** 4 / 3456
    s = np.sqrt(np.where(small, 1.0, s2))
    th = np.arctan2(s.real, c.real)
    if np.iscomplexobj(Q):
        th = th + 1j * (c.real * s.imag - s.real * c.imag) / (c.real ** 2 + s.real ** 2)
    k = np.where(small, ser, th / s)
    return 0.5 * k[..., None] * v


def between(za, zb, rel=None):
    """e [..., 6] of the pair of poses za, zb [..., 6] (real or complex), rel [6] or None"""
    za, zb = np.asarray(za), np.asarray(zb)
    Ra, Rb = tr.rodrigues(za[..., :3]), tr.rodrigues(zb[..., :3])
    dt = 0.0
    if rel is not None:
        rel = np.asarray(rel, dtype=np.float64)
        Ra = Ra @ tr.rodrigues(rel[:3])
        dt = rel[3:]
    Q = np.swapaxes(Ra, -1, -2) @ Rb
    return np.concatenate([so3_log(Q), zb[..., 3:] - za[..., 3:] - dt], -1)


def between_jacobian(za, zb, rel=None, h=H_CS):
    """(J [6, 12] = d e / d (za, zb) by complex step, e [6]) at the real poses"""
    za, zb = np.asarray(za, dtype=np.float64), np.asarray(zb, dtype=np.float64)
    x = np.concatenate([za, zb])[None, :] + 1j * h * np.eye(12)
    ec = between(x[:, :6], x[:, 6:], rel)          # [12, 6]
    return (ec.imag / h).T, between(za, zb, rel)


class SmoothProblem:
    """the joint problem over a TrackData: delta < 0 / None = no Huber weights"""

    def __init__(self, td, sigma_rot, sigma_trans, delta=-1.0, frame_time=None, rel_motion=None):
        self.td, self.F = td, td.F
        self.delta = -1.0 if delta is None else delta
        F = td.F
        dt = np.ones(max(F - 1, 0)) if frame_time is None else np.diff(np.asarray(frame_time, dtype=np.float64))
        self.lam = np.zeros((max(F - 1, 0), 6))
        self.lam[:, :3] = (1.0 / (sigma_rot * sigma_rot * dt))[:, None]
        self.lam[:, 3:] = (1.0 / (sigma_trans * sigma_trans * dt))[:, None]
        self.rel = None if rel_motion is None else np.asarray(rel_motion, dtype=np.float64).reshape(F - 1, 6)
        self.fd = [td.frame(f) for f in range(F)]
        self.rows = 8.0 * float(td.start[F] - td.start[0]) + 6.0 * (F - 1)

    def _rel(self, f):
        return None if self.rel is None else self.rel[f]

    def costs(self, z):
        """(data cost per frame [F], prior cost per pair [F-1]) at z [F, 6]"""
        Ef = np.array([tr.frame_error(self.fd[f], z[f], self.delta) for f in range(self.F)])
        if self.F > 1:
            e = np.stack([between(z[f], z[f + 1], self._rel(f)) for f in range(self.F - 1)])
            Pe = np.sum(self.lam * e * e, axis=1)
        else:
            Pe = np.zeros(0)
        return Ef, Pe

    def cost(self, z):
        Ef, Pe = self.costs(z)
        return float(np.sum(Ef) + np.sum(Pe))

    def system(self, z):
        """(diag [F, 6, 6], off [F-1, 6, 6], rhs [6F]) at z [F, 6]"""
        F = self.F
        diag, off, rhs = np.zeros((F, 6, 6)), np.zeros((max(F - 1, 0), 6, 6)), np.zeros((F, 6))
        for f in range(F):
            J, rw = tr.jacobian(self.fd[f], z[f], self.delta)
            diag[f] = J.T @ J
            rhs[f] = -J.T @ rw
        for f in range(F - 1):
            J, e = between_jacobian(z[f], z[f + 1], self._rel(f))
            L = self.lam[f]
            Ja, Jb = J[:, :6], J[:, 6:]
            diag[f] += Ja.T @ (L[:, None] * Ja)
            diag[f + 1] += Jb.T @ (L[:, None] * Jb)
            off[f] = Ja.T @ (L[:, None] * Jb)
            rhs[f] -= Ja.T @ (L * e)
            rhs[f + 1] -= Jb.T @ (L * e)
        return diag, off, rhs.reshape(-1)


def dense(diag, off):
    F = diag.shape[0]
    H = np.zeros((6 * F, 6 * F), dtype=diag.dtype)
    for f in range(F):
        H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = diag[f]
    for f in range(F - 1):
        H[6 * f:6 * f + 6, 6 * f + 6:6 * f + 12] = off[f]
        H[6 * f + 6:6 * f + 12, 6 * f:6 * f + 6] = off[f].T
    return H


def banded(diag, off, mu=0.0):
    """lower banded storage ab[i - j, j] (12 rows) of H + mu I"""
    F = diag.shape[0]
    n = 6 * F
    ab = np.zeros((12, n), dtype=diag.dtype)
    for r in range(6):
        for c in range(r + 1):
            ab[r - c, c:n:6] = diag[:, r, c]          # entries (6f + r, 6f + c)
    ab[0] += mu
    for r in range(6):          # row r of frame f + 1, column c of frame f: off[f][c][r]
        for c in range(6):
            ab[6 + r - c, c:n - 6:6] = off[:, c, r]
    return ab


def solve(diag, off, rhs, mu):
    if diag.shape[0] == 0:
        return np.zeros(0)
    if solveh_banded is not None:
        return solveh_banded(banded(diag, off, mu), rhs, lower=True)
    return np.linalg.solve(dense(diag, off) + mu * np.eye(rhs.size), rhs)


def matvec(diag, off, x, mu=0.0):
    """(H + mu I) x from the blocks"""
    F = diag.shape[0]
    X = np.asarray(x).reshape(F, 6)
    Y = np.einsum("fij,fj->fi", diag, X) + mu * X
    if F > 1:
        Y[:-1] += np.einsum("fij,fj->fi", off, X[1:])
        Y[1:] += np.einsum("fji,fj->fi", off, X[:-1])
    return Y.reshape(-1)


def smooth_lm(sp, z0, max_iters=10000, min_error=1e-5, min_step=0.0, min_avg=1e-4, tau=1.0):
    """aar_track_smooth's loop from the poses z0 [F, 6].  Returns a dict: z, iterations, err, data, prior, exit, rejected, mu, margin, slack
    (margin / slack as in track_restated.track_frame, over the joint run), grad0 / grad (|b|_inf at the start and at the result)."""
    z = np.array(z0, dtype=np.float64).reshape(sp.F, 6)
    rows = sp.rows
    Ef, Pe = sp.costs(z) if sp.F else (np.zeros(0), np.zeros(0))
    data, prior = float(np.sum(Ef)), float(np.sum(Pe))
    curr = data + prior
    prev = curr
    mu, v = -1.0, 2.0
    must, iters, rejected = 0, 0, 0
    margin, slack = np.inf, 0.0
    it = 0
    grad0 = None
    while it < max_iters and not must and rows > 0 and sp.F > 0:
        diag, off, B = sp.system(z)
        if grad0 is None:
            grad0 = float(np.abs(B).max())
        if mu < 0:
            mu = float(np.max(np.einsum("fii->fi", diag))) * tau
        ntries, accepted = 0, False
        while True:
            d = solve(diag, off, B, mu)
            zt = z + d.reshape(sp.F, 6)
            Ef, Pe = sp.costs(zt)
            err = float(np.sum(Ef) + np.sum(Pe))
            d2, dg = float(d @ d), float(d @ B)
            Lq = 0.5 * (mu * d2 - dg)
            with np.errstate(divide="ignore", invalid="ignore"):
                gain = float(np.float64(err - prev) / np.float64(Lq))
            if abs(err - prev) > 0.5 * rows * min_avg:
                margin = min(margin, tr._margin(err, prev, max(err, prev)), tr._margin(mu * d2, dg, abs(mu * d2) + abs(dg)))
            if tr._margin(err, prev, max(err, prev)) <= MARGIN:
                slack = max(slack, float(np.abs(d).max()))
            if gain > 0 and err - prev < 0:
                t = 2 * gain - 1
                mu = mu * max(0.33, 1.0 - t * t * t)
                v = 2.0
                curr, data, prior = err, float(np.sum(Ef)), float(np.sum(Pe))
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
        margin = min(margin, tr._margin(curr, min_error, max(curr, min_error)))
        dd = abs(prev - curr)
        if dd <= min_step or abs((prev - curr) / rows) <= min_avg or not accepted:
            must = 2
        margin = min(margin, tr._margin(dd, min_step, max(scale, min_step)) if min_step > 0 else np.inf,
                     tr._margin(dd, rows * min_avg, max(scale, rows * min_avg)))
        if curr > prev:
            must = 3
        iters += 1
        prev = curr
        it += 1
    grad = float(np.abs(sp.system(z)[2]).max()) if sp.F else 0.0
    return dict(z=z, iterations=iters, err=curr, data=data, prior=prior, exit=must, rejected=rejected, mu=mu, margin=margin, slack=slack,
                grad0=grad if grad0 is None else grad0, grad=grad)


def geodesic(za, zb, s):
    """the pose a fraction s of the way from za to zb: R_a Exp(s log(R_a^T R_b)), t_a + s (t_b - t_a), as a 6-vector (rvec, t)"""
    Ra, Rb = tr.rodrigues(za[:3]), tr.rodrigues(zb[:3])
    R = Ra @ tr.rodrigues(s * so3_log(Ra.T @ Rb))
    return np.concatenate([so3_log(R), za[3:] + s * (zb[3:] - za[3:])])
