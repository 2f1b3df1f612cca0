"""float64 restatement of the live tracker's constant-velocity motion model -- TEST INFRASTRUCTURE ONLY.

Built on tests/live_restated.py, tests/live_marginal_restated.py, tests/smooth_restated.py and tests/track_restated.py (imported, not edited),
independent of csrc/live_kernels.hip and host/motion_model.h:

    rel          every window frame i carries the expected motion rel[i] (rvec, t) of the pair that ENDS at it (i = 0: the anchor pair); the pair's
                 error is smooth_restated.between(z_{i-1}, z_i, rel[i]), its Jacobian between_jacobian(..., rel[i]) (complex step)
    marginal     live_marginal_restated's, with pair (0, 1) taken with rel[1]: B = J_b^T L_1 J_b, c = -J_b^T L_1 e_0
    measure      rel_n and the prediction from the two newest estimates (a, b) and the three times:
                     omega = log(R_a^T R_b), v = t_b - t_a, s = (time_n - time_b) / (time_b - time_a), rel_n = (s omega, s v),
                     prediction = (R_b exp(s omega), t_b + s v); zero / z_b before two frames or, with max_dt > 0, when a gap exceeds it
    driver       LiveCV: live_marginal_restated.LiveM's push loop with the rule above: rel_n is measured when frame n is pushed and stays with it
"""
import numpy as np

import live_marginal_restated as lm
import live_restated as lr
import smooth_restated as sr
import track_restated as tr


def measure(za, zb, ta, tb, time, max_dt=0.0):
    """(rel [6], prediction [6], predicted) of the frame pushed at `time` from the estimates za (None: fewer than two frames), zb at ta, tb"""
    zb = np.asarray(zb, dtype=np.float64)
    if za is None or (max_dt > 0.0 and (tb - ta > max_dt or time - tb > max_dt)):
        return np.zeros(6), zb.copy(), False
    za = np.asarray(za, dtype=np.float64)
    Ra, Rb = tr.rodrigues(za[:3]), tr.rodrigues(zb[:3])
    s = (time - tb) / (tb - ta)
    rel = s * np.concatenate([sr.so3_log(Ra.T @ Rb), zb[3:] - za[3:]])
    pred = np.concatenate([sr.so3_log(Rb @ tr.rodrigues(rel[:3])), zb[3:] + rel[3:]])
    return rel, pred, True


def velocity(za, zb, ta, tb):
    """(omega, v) per unit of time of the pair (a, b)"""
    za, zb = np.asarray(za, dtype=np.float64), np.asarray(zb, dtype=np.float64)
    return np.concatenate([sr.so3_log(tr.rodrigues(za[:3]).T @ tr.rodrigues(zb[:3])), zb[3:] - za[3:]]) / (tb - ta)


def predict(zb, vel, tb, time, max_dt=0.0):
    """the pose zb at tb carried to time >= tb with vel; zb itself past max_dt (> 0)"""
    zb = np.asarray(zb, dtype=np.float64)
    d = time - tb
    assert d >= 0
    if max_dt > 0.0 and d > max_dt:
        return zb.copy()
    return np.concatenate([sr.so3_log(tr.rodrigues(zb[:3]) @ tr.rodrigues(d * vel[:3])), zb[3:] + d * vel[3:]])


class WindowProblemCV(lm.WindowProblemM):
    """live_marginal_restated.WindowProblemM with rel [W, 6]: the expected motion of the pair that ends at each window frame"""

    def __init__(self, td, frames, times, sigma_rot=1.0, sigma_trans=1.0, delta=-1.0, anchor=None, smooth=True, prior=None, rel=None):
        super().__init__(td, frames, times, sigma_rot, sigma_trans, delta, anchor=anchor, smooth=smooth, prior=prior)
        self.rel = np.zeros((self.F, 6)) if rel is None else np.array(rel, dtype=np.float64).reshape(self.F, 6)

    def _pairs(self):
        """the window positions that carry a pair"""
        return [i for i in range(self.F) if self.smooth and (i > 0 or self.anchor is not None)]

    def costs(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(self.F, 6)
        Ef = np.array([tr.frame_error(self.fd[i], z[i], self.delta) for i in range(self.F)])
        Pe = np.zeros(self.F)
        for i in self._pairs():
            e = sr.between(self.anchor if i == 0 else z[i - 1], z[i], self.rel[i])
            Pe[i] = float(np.sum(self.lam[i] * e * e))
        if self.prior is not None:
            e = z[0] - self.prior[1]
            Pe[0] = float(e @ self.prior[0] @ e)
        return Ef, Pe

    def cost(self, z):
        Ef, Pe = self.costs(z)
        return float(np.sum(Ef) + np.sum(Pe))

    def cost_complex(self, zc):
        """the cost at a complex point (no Huber weights): for the complex-step derivative of the tests"""
        assert self.delta < 0
        zc = np.asarray(zc).reshape(self.F, 6)
        E = 0.0
        for i in range(self.F):
            r = tr.residuals(self.fd[i], zc[i])
            E = E + np.sum(r * r)
        for i in self._pairs():
            e = sr.between(self.anchor.astype(complex) if i == 0 else zc[i - 1], zc[i], self.rel[i])
            E = E + np.sum(self.lam[i] * e * e)
        if self.prior is not None:
            e = zc[0] - self.prior[1]
            E = E + e @ self.prior[0] @ e
        return E

    def system(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(self.F, 6)
        F = self.F
        diag, off, rhs = np.zeros((F, 6, 6)), np.zeros((max(F - 1, 0), 6, 6)), np.zeros((F, 6))
        for i in range(F):
            J, rw = tr.jacobian(self.fd[i], z[i], self.delta)
            diag[i] = J.T @ J
            rhs[i] = -J.T @ rw
        for i in self._pairs():
            J, e = sr.between_jacobian(self.anchor if i == 0 else z[i - 1], z[i], self.rel[i])
            L = self.lam[i]
            Ja, Jb = J[:, :6], J[:, 6:]
            diag[i] += Jb.T @ (L[:, None] * Jb)
            rhs[i] -= Jb.T @ (L * e)
            if i > 0:
                diag[i - 1] += Ja.T @ (L[:, None] * Ja)
                off[i - 1] = Ja.T @ (L[:, None] * Jb)
                rhs[i - 1] -= Ja.T @ (L * e)
        if self.prior is not None:
            diag[0] += self.prior[0]
            rhs[0] -= self.prior[0] @ (z[0] - self.prior[1])
        return diag, off, rhs.reshape(-1)


def marginal_terms(wp, z):
    """(L', b', B) of the first window frame marginalised at z [W, 6] (W >= 2), pair (0, 1) with its expected motion"""
    z = np.asarray(z, dtype=np.float64).reshape(wp.F, 6)
    diag, off, rhs = wp.system(z)
    A, a, O = diag[0], rhs[:6], off[0]
    J, e = sr.between_jacobian(z[0], z[1], wp.rel[1])
    L = wp.lam[1]
    Jb = J[:, 6:]
    B = Jb.T @ (L[:, None] * Jb)
    c = -Jb.T @ (L * e)
    Ai = np.linalg.inv(A)
    return B - O.T @ Ai @ O, c - O.T @ Ai @ a, B


def marginalise(wp, z):
    """the prior (L', m') the next push puts on window frame 1, or None when L' is dropped (live_marginal_restated's rule)"""
    z = np.asarray(z, dtype=np.float64).reshape(wp.F, 6)
    Lp, bp, B = marginal_terms(wp, z)
    d = lm.ldl_pivots(Lp)
    if not np.all(d > lm.PIVOT_REL * np.diag(B)):
        return None
    Lp = 0.5 * (Lp + Lp.T)
    return Lp, z[1] + np.linalg.inv(Lp) @ bp


class LiveCV:
    """push-by-push driver with the constant-velocity model: live_marginal_restated.LiveM's loop, window entries [frame, time, pose, rel];
    model = False: the random walk (rel = 0, the start is the previous estimate) through the same code"""

    def __init__(self, td, lag=0, sigma_rot=1.0, sigma_trans=1.0, delta=-1.0, anchor="fixed", max_dt=0.0, model=True, **lmkw):
        assert 0 <= lag <= 15 and anchor in ("fixed", "marginal") and (anchor == "fixed" or lag >= 1)
        self.td, self.lag, self.sr, self.st, self.delta, self.lmkw = td, lag, sigma_rot, sigma_trans, delta, lmkw
        self.marginal, self.max_dt, self.model = anchor == "marginal", float(max_dt), bool(model)
        self.reset()

    def reset(self):
        self.n = 0
        self.win = []
        self.anchor = None     # (pose, time)
        self.prior = None
        self.dropped = 0

    def newest_pair(self):
        """(za or None, zb, ta, tb) as the last push left them"""
        if not self.win:
            return None, None, None, None
        b = self.win[-1]
        if len(self.win) >= 2:
            a = self.win[-2]
            return a[2], b[2], a[1], b[1]
        if self.anchor is not None:
            return self.anchor[0], b[2], self.anchor[1], b[1]
        return None, b[2], None, b[1]

    def push(self, f, time, pose_init=None):
        """LiveM.push's dict plus rel (of this push), predicted, prediction (None on the first push), velocity (after the push)"""
        za, zb, ta, tb = self.newest_pair()
        rel, pred, predicted = np.zeros(6), None, False
        if zb is not None:
            rel, pred, predicted = measure(za, zb, ta, tb, time, self.max_dt) if self.model else (np.zeros(6), zb.copy(), False)
        if pose_init is None:
            assert self.win, "the first push needs a pose_init"
            start = pred.copy()
        else:
            start = np.array(pose_init, dtype=np.float64)
        assert not self.win or time > self.win[-1][1]
        left = None
        if len(self.win) == self.lag + 1:
            left = self.win.pop(0)
            self.anchor = (left[2], left[1])
        self.win.append([f, float(time), start, rel])
        wp = WindowProblemCV(self.td, [w[0] for w in self.win], [w[1] for w in self.win], self.sr, self.st, self.delta,
                             anchor=None if self.marginal else self.anchor, smooth=True, prior=self.prior if self.marginal else None,
                             rel=np.stack([w[3] for w in self.win]))
        z0 = np.stack([w[2] for w in self.win])
        r = lr.push_lm(wp, z0, **self.lmkw)
        for w, z in zip(self.win, r["z"]):
            w[2] = np.array(z)
        full = len(self.win) == self.lag + 1
        zf = np.stack([w[2] for w in self.win])
        prior_in = self.prior
        if self.marginal and full:
            self.prior = marginalise(wp, zf)
            if self.prior is None:
                self.dropped += 1
        cov, valid = lm.cov_blocks(wp, zf)
        za, zb, ta, tb = self.newest_pair()
        r.update(frame_index=self.n, window_frames=len(self.win), pose=self.win[-1][2].copy(),
                 lagged_pose=self.win[0][2].copy() if full else None, problem=wp, prior_in=prior_in,
                 marginal=self.prior if self.marginal else None, has_marginal=int(self.marginal and self.prior is not None),
                 marginal_index=(self.n - len(self.win) + 2) if (self.marginal and self.prior is not None) else -1, dropped=self.dropped,
                 cov=cov, cov_valid=int(valid), sigma2=lm.sigma2(r["err"], wp.rows, len(self.win)), start=z0, left=left,
                 rel=rel, predicted=int(predicted), prediction=pred, initial=wp.cost(z0),
                 velocity=np.zeros(6) if za is None else velocity(za, zb, ta, tb))
        self.n += 1
        return r

    def window(self):
        return np.stack([w[2] for w in self.win]), (None if self.anchor is None else self.anchor[0])
