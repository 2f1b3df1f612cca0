"""float64 restatement of smoothed tracking under the constant-velocity prior (aar_track_smooth with AAR_SMOOTH_MODEL_CONSTANT_VELOCITY,
DESIGN.md section 31) -- TEST INFRASTRUCTURE ONLY.

Built on tests/smooth_restated.py and tests/track_restated.py (imported, not edited) and independent of csrc/smooth_cv_kernels.hip:

    cost         E(z) = sum_f E_f(z_f) + e_0^T L_0 e_0 + sum_{1 <= f <= F-2} e_f^T L_f e_f
    pair 0       e_0 = smooth_restated.between(z_0, z_1),  L_0 = L(sigma_rot0, sigma_trans0, D_0)
    term f       e_f = [ log((R_f dR_f)^T R_{f+1})^v ; t_{f+1} - t_f - r_f (t_f - t_{f-1}) ],  dR_f = Exp(r_f log(R_{f-1}^T R_f)),
                 r_f = D_f / D_{f-1},  L_f = L(sigma_rot, sigma_trans, D_f),  L(sr, st, D) = diag(1 / (sr^2 D) x3, 1 / (st^2 D) x3)
    Jacobian     complex step on e_f over the eighteen entries of (z_{f-1}, z_f, z_{f+1}), h = 1e-30: no analytic derivation; the
                 dependence of dR_f on z_{f-1}, z_f is differentiated with everything else
    system       block pentadiagonal: diag [F], off [F-1] = H_{f,f+1}, off2 [F-2] = H_{f,f+2}, rhs
    solve        scipy.linalg.solveh_banded with 18 sub-diagonals (numpy.linalg.solve on the dense matrix without scipy)
    LM           smooth_restated.smooth_lm's loop, rows = 8 N + 6 (F - 1)
"""
import numpy as np

import smooth_restated as sr
import track_restated as tr

try:
    from scipy.linalg import solveh_banded
except ImportError:   # pragma: no cover
    solveh_banded = None

H_CS = tr.H_CS
MARGIN = tr.MARGIN


def cv_term(zp, zc, zn, r):
    """e [..., 6] of the term over the poses of frames f-1, f, f+1 (real or complex), r = D_f / D_{f-1}"""
    zp, zc, zn = np.asarray(zp), np.asarray(zc), np.asarray(zn)
    Rp, Rc, Rn = tr.rodrigues(zp[..., :3]), tr.rodrigues(zc[..., :3]), tr.rodrigues(zn[..., :3])
    psi = sr.so3_log(np.swapaxes(Rp, -1, -2) @ Rc)
    dR = tr.rodrigues(r * psi)
    Q = np.swapaxes(Rc @ dR, -1, -2) @ Rn
    return np.concatenate([sr.so3_log(Q), zn[..., 3:] - zc[..., 3:] - r * (zc[..., 3:] - zp[..., 3:])], -1)


def cv_term_jacobian(zp, zc, zn, r, h=H_CS):
    """(J [6, 18] = d e / d (zp, zc, zn) by complex step, e [6]) at the real poses"""
    z = np.concatenate([np.asarray(zp, dtype=np.float64), np.asarray(zc, dtype=np.float64), np.asarray(zn, dtype=np.float64)])
    x = z[None, :] + 1j * h * np.eye(18)
    ec = cv_term(x[:, :6], x[:, 6:12], x[:, 12:], r)          # [18, 6]
    return (ec.imag / h).T, cv_term(z[:6], z[6:12], z[12:], r)


class SmoothCvProblem:
    """the joint problem over a TrackData under the constant-velocity prior: delta < 0 / None = no Huber weights"""

    def __init__(self, td, sigma_rot, sigma_trans, sigma_rot0, sigma_trans0, delta=-1.0, frame_time=None):
        self.td, self.F = td, td.F
        self.delta = -1.0 if delta is None else delta
        F = td.F
        dt = np.ones(max(F - 1, 0)) if frame_time is None else np.diff(np.asarray(frame_time, dtype=np.float64))
        self.lam = np.zeros((max(F - 1, 0), 6))          # entry 0: pair 0, entry f: term f
        self.ratio = np.zeros(max(F - 1, 0))
        if F > 1:
            self.lam[:, :3] = (1.0 / (sigma_rot * sigma_rot * dt))[:, None]
            self.lam[:, 3:] = (1.0 / (sigma_trans * sigma_trans * dt))[:, None]
            self.lam[0, :3] = 1.0 / (sigma_rot0 * sigma_rot0 * dt[0])
            self.lam[0, 3:] = 1.0 / (sigma_trans0 * sigma_trans0 * dt[0])
            self.ratio[1:] = dt[1:] / dt[:-1]
        self.fd = [td.frame(f) for f in range(F)]
        self.rows = 8.0 * float(td.start[F] - td.start[0]) + 6.0 * (F - 1)

    def prior_errors(self, z):
        """e [F-1, 6]: pair 0, then the terms 1 .. F-2"""
        F = self.F
        if F < 2:
            return np.zeros((0, 6))
        e = [sr.between(z[0], z[1])]
        e += [cv_term(z[f - 1], z[f], z[f + 1], self.ratio[f]) for f in range(1, F - 1)]
        return np.stack(e)

    def costs(self, z):
        """(data cost per frame [F], prior cost per term [F-1]) at z [F, 6]"""
        Ef = np.array([tr.frame_error(self.fd[f], z[f], self.delta) for f in range(self.F)])
        e = self.prior_errors(z)
        return Ef, np.sum(self.lam * e * e, axis=1)

    def cost(self, z):
        Ef, Pe = self.costs(z)
        return float(np.sum(Ef) + np.sum(Pe))

    def system(self, z):
        """(diag [F, 6, 6], off [F-1, 6, 6], off2 [F-2, 6, 6], rhs [6F]) at z [F, 6]"""
        F = self.F
        H = {}
        rhs = np.zeros((F, 6))
        for f in range(F):
            J, rw = tr.jacobian(self.fd[f], z[f], self.delta)
            H[f, f] = J.T @ J
            rhs[f] = -J.T @ rw
        for f in range(F - 1):
            if f == 0:
                J, e = sr.between_jacobian(z[0], z[1])
                frames = (0, 1)
            else:
                J, e = cv_term_jacobian(z[f - 1], z[f], z[f + 1], self.ratio[f])
                frames = (f - 1, f, f + 1)
            L = self.lam[f]
            for a, fa in enumerate(frames):
                Ja = J[:, 6 * a:6 * a + 6]
                rhs[fa] -= Ja.T @ (L * e)
                for b, fb in enumerate(frames):
                    if fb >= fa:
                        H[fa, fb] = H.get((fa, fb), 0.0) + Ja.T @ (L[:, None] * J[:, 6 * b:6 * b + 6])
        z6 = np.zeros((6, 6))
        diag = np.stack([H[f, f] for f in range(F)]) if F else np.zeros((0, 6, 6))
        off = np.stack([H.get((f, f + 1), z6) for f in range(F - 1)]) if F > 1 else np.zeros((0, 6, 6))
        off2 = np.stack([H.get((f, f + 2), z6) for f in range(F - 2)]) if F > 2 else np.zeros((0, 6, 6))
        return diag, off, off2, rhs.reshape(-1)


def dense(diag, off, off2):
    F = diag.shape[0]
    H = sr.dense(diag, off)
    for f in range(F - 2):
        H[6 * f:6 * f + 6, 6 * f + 12:6 * f + 18] = off2[f]
        H[6 * f + 12:6 * f + 18, 6 * f:6 * f + 6] = off2[f].T
    return H


def banded(diag, off, off2, mu=0.0):
    """lower banded storage ab[i - j, j] (18 rows) of H + mu I"""
    F = diag.shape[0]
    n = 6 * F
    ab = np.zeros((18, n), dtype=diag.dtype)
    ab[:12] = sr.banded(diag, off, mu)
    for r in range(6):          # row r of frame f + 2, column c of frame f: off2[f][c][r]
        for c in range(6):
            ab[12 + r - c, c:max(n - 12, 0):6] = off2[:, c, r]
    return ab


def solve(diag, off, off2, rhs, mu, use_banded=True):
    if diag.shape[0] == 0:
        return np.zeros(0)
    if use_banded and solveh_banded is not None:
        return solveh_banded(banded(diag, off, off2, mu), rhs, lower=True)
    return np.linalg.solve(dense(diag, off, off2) + mu * np.eye(rhs.size), rhs)


def matvec(diag, off, off2, x, mu=0.0):
    """(H + mu I) x from the blocks"""
    F = diag.shape[0]
    X = np.asarray(x).reshape(F, 6)
    Y = sr.matvec(diag, off, x, mu).reshape(F, 6)
    if F > 2:
        Y[:-2] += np.einsum("fij,fj->fi", off2, X[2:])
        Y[2:] += np.einsum("fji,fj->fi", off2, X[:-2])
    return Y.reshape(-1)


def smooth_lm(sp, z0, max_iters=10000, min_error=1e-5, min_step=0.0, min_avg=1e-4, tau=1.0):
    """aar_track_smooth's loop from the poses z0 [F, 6]: smooth_restated.smooth_lm line for line, on the pentadiagonal system.  Returns the
    same dict."""
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
        diag, off, off2, B = sp.system(z)
        if grad0 is None:
            grad0 = float(np.abs(B).max())
        if mu < 0:
            mu = float(np.max(np.einsum("fii->fi", diag))) * tau
        ntries, accepted = 0, False
        while True:
            d = solve(diag, off, off2, B, mu)
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
    grad = float(np.abs(sp.system(z)[3]).max()) if sp.F else 0.0
    return dict(z=z, iterations=iters, err=curr, data=data, prior=prior, exit=must, rejected=rejected, mu=mu, margin=margin, slack=slack,
                grad0=grad if grad0 is None else grad0, grad=grad)
