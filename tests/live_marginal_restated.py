"""float64 restatement of the live tracker's marginalised anchor and per-push covariance -- TEST INFRASTRUCTURE ONLY.

Built on tests/live_restated.py, tests/smooth_restated.py and tests/track_restated.py (imported, not edited), independent of csrc/live_kernels.hip:

    prior        E_m(z_0) = (z_0 - m)^T Lm (z_0 - m) on the first window frame in place of the anchor pair: D_0 += Lm, b_0 -= Lm (z_0 - m),
                 Pe[0] = E_m, 6 rows
    marginal     at the final point of a push with a full window, from the system there (mu = 0): A = D_0, a = b_0, O = O_0 and the J_b half of
                 pair (0, 1) alone, B = J_b^T L_1 J_b, c = -J_b^T L_1 e_0 (complex-step J_b):
                     L' = B - O^T A^-1 O,  b' = c - O^T A^-1 a,  m' = z_1 + L'^-1 b'
                 L' is dropped when a pivot of its LDL^T is not above PIVOT_REL times the matching diagonal entry of B (an exact 0 -- a leaving
                 frame with neither prior nor detections -- is rounding noise of either sign in floating point)
    covariance   numpy.linalg.inv of the dense window H, its diagonal 6x6 blocks; sigma2 = cost / (rows - 6 W), 0 when rows <= 6 W
    driver       LiveM: live_restated.Live's push loop with anchor = "fixed" | "marginal"
"""
import numpy as np

import live_restated as lr
import smooth_restated as sr

PIVOT_REL = 1e-10


class WindowProblemM(lr.WindowProblem):
    """live_restated.WindowProblem plus prior = (Lm [6, 6], m [6]) on the first window frame (None: none).  With a prior there is no anchor."""

    def __init__(self, td, frames, times, sigma_rot=1.0, sigma_trans=1.0, delta=-1.0, anchor=None, smooth=True, prior=None):
        assert prior is None or (anchor is None and smooth)
        super().__init__(td, frames, times, sigma_rot, sigma_trans, delta, anchor=anchor, smooth=smooth)
        self.prior = None if prior is None else (np.array(prior[0], dtype=np.float64), np.array(prior[1], dtype=np.float64))
        if self.prior is not None:
            self.rows += 6.0

    def costs(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(self.F, 6)
        Ef, Pe = super().costs(z)
        if self.prior is not None:
            e = z[0] - self.prior[1]
            Pe[0] = float(e @ self.prior[0] @ e)
        return Ef, Pe

    def cost(self, z):
        Ef, Pe = self.costs(z)
        return float(np.sum(Ef) + np.sum(Pe))

    def system(self, z):
        z = np.asarray(z, dtype=np.float64).reshape(self.F, 6)
        diag, off, rhs = super().system(z)
        if self.prior is not None:
            diag[0] += self.prior[0]
            rhs[:6] -= self.prior[0] @ (z[0] - self.prior[1])
        return diag, off, rhs


def ldl_pivots(S):
    """the pivots of the LDL^T elimination of a symmetric matrix, in order, without pivoting"""
    a = np.array(S, dtype=np.float64)
    n = a.shape[0]
    d = np.zeros(n)
    for p in range(n):
        d[p] = a[p, p]
        if d[p] == 0.0 or not np.isfinite(d[p]):
            d[p + 1:] = np.nan
            break
        a[p + 1:, p + 1:] -= np.outer(a[p + 1:, p], a[p, p + 1:]) / d[p]
    return d


def marginal_terms(wp, z):
    """(L', b', B) of the first window frame marginalised at z [W, 6] (W >= 2)"""
    z = np.asarray(z, dtype=np.float64).reshape(wp.F, 6)
    diag, off, rhs = wp.system(z)
    A, a, O = diag[0], rhs[:6], off[0]
    J, e = sr.between_jacobian(z[0], z[1])
    L = wp.lam[1]
    Jb = J[:, 6:]
    B = Jb.T @ (L[:, None] * Jb)
    c = -Jb.T @ (L * e)
    Ai = np.linalg.inv(A)
    return B - O.T @ Ai @ O, c - O.T @ Ai @ a, B


def pivot_ratios(wp, z):
    """the pivots of L' over the matching diagonal entries of B: what marginalise holds against PIVOT_REL"""
    Lp, _, B = marginal_terms(wp, z)
    return ldl_pivots(Lp) / np.diag(B)


def marginalise(wp, z):
    """the prior (L', m') the next push puts on window frame 1, or None when L' is dropped"""
    z = np.asarray(z, dtype=np.float64).reshape(wp.F, 6)
    Lp, bp, B = marginal_terms(wp, z)
    d = ldl_pivots(Lp)
    if not np.all(d > PIVOT_REL * np.diag(B)):      # (a NaN pivot compares false)
        return None
    Lp = 0.5 * (Lp + Lp.T)
    return Lp, z[1] + np.linalg.inv(Lp) @ bp


def cov_blocks(wp, z):
    """(the diagonal 6x6 blocks [W, 6, 6] of inv(H) at z, valid): H the dense window system; invalid (zeros) when H is not positive definite"""
    z = np.asarray(z, dtype=np.float64).reshape(wp.F, 6)
    diag, off, _ = wp.system(z)
    H = sr.dense(diag, off)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return np.zeros((wp.F, 6, 6)), False
    Hi = np.linalg.inv(H)
    return np.stack([Hi[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(wp.F)]), True


def sigma2(cost, rows, W):
    return cost / (rows - 6.0 * W) if rows > 6.0 * W else 0.0


class LiveM:
    """push-by-push driver: live_restated.Live with anchor = "fixed" | "marginal" and the uncertainty record after every push"""

    def __init__(self, td, lag=0, smooth=False, sigma_rot=1.0, sigma_trans=1.0, delta=-1.0, anchor="fixed", **lm):
        assert 0 <= lag <= 15 and (smooth or lag == 0) and anchor in ("fixed", "marginal")
        assert anchor == "fixed" or (smooth and lag >= 1)
        self.td, self.lag, self.smooth, self.sr, self.st, self.delta, self.lm = td, lag, bool(smooth), sigma_rot, sigma_trans, delta, lm
        self.marginal = anchor == "marginal"
        self.reset()

    def reset(self):
        self.n = 0
        self.win = []          # [frame of td, time, pose] oldest first
        self.anchor = None     # (pose, time): kept in both modes
        self.prior = None      # (Lm, m) on the first frame of the NEXT push's window
        self.dropped = 0

    def problem(self, win=None, prior="own"):
        win = self.win if win is None else win
        return WindowProblemM(self.td, [w[0] for w in win], [w[1] for w in win], self.sr, self.st, self.delta,
                              anchor=None if self.marginal else self.anchor, smooth=self.smooth,
                              prior=(self.prior if prior == "own" else prior) if self.marginal else None)

    def push(self, f, time, pose_init=None):
        """live_restated.Live.push's dict plus prior_in (the prior this push used), marginal (the one it leaves, or None), has_marginal,
        marginal_index, dropped (so far), cov [W, 6, 6], cov_valid, sigma2, start [W, 6] and left = [frame, time, pose] of the frame that
        left the window at this push (None while it fills)"""
        if pose_init is None:
            assert self.win, "the first push needs a pose_init"
            start = self.win[-1][2].copy()
        else:
            start = np.array(pose_init, dtype=np.float64)
        assert not self.win or time > self.win[-1][1]
        left = None
        if len(self.win) == self.lag + 1:
            left = self.win.pop(0)
            self.anchor = (left[2], left[1])
        self.win.append([f, float(time), start])
        wp = self.problem()
        z0 = np.stack([w[2] for w in self.win])
        r = lr.push_lm(wp, z0, **self.lm)
        for w, z in zip(self.win, r["z"]):
            w[2] = np.array(z)
        full = len(self.win) == self.lag + 1
        zf = np.stack([w[2] for w in self.win])
        prior_in = self.prior
        if self.marginal and full:
            self.prior = marginalise(wp, zf)
            if self.prior is None:
                self.dropped += 1
        cov, valid = cov_blocks(wp, zf)
        r.update(frame_index=self.n, window_frames=len(self.win), pose=self.win[-1][2].copy(),
                 lagged_pose=self.win[0][2].copy() if full else None, problem=wp, prior_in=prior_in,
                 marginal=self.prior if self.marginal else None, has_marginal=int(self.marginal and self.prior is not None),
                 marginal_index=(self.n - len(self.win) + 2) if (self.marginal and self.prior is not None) else -1, dropped=self.dropped,
                 cov=cov, cov_valid=int(valid), sigma2=sigma2(r["err"], wp.rows, len(self.win)), start=z0, left=left)
        self.n += 1
        return r

    def window(self):
        return np.stack([w[2] for w in self.win]), (None if self.anchor is None else self.anchor[0])
