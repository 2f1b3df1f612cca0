"""float64 restatement of the live tracker (aar_tracker_push) -- TEST INFRASTRUCTURE ONLY.

Built on tests/track_restated.py and tests/smooth_restated.py (imported, not edited) and independent of csrc/live_kernels.hip:

    window       after push n the last W = min(n + 1, lag + 1) pushed frames; the frame that left last is the anchor, a constant
    cost         E = sum_{f in window} E_f(z_f) + sum_{f, f+1 in window} e_f^T L_f e_f + [anchor] e_a^T L_a e_a,  e_a = between(z_anchor, z_first),
                 L from the pushes' times; smooth = 0: the data term of one frame alone
    system       H, b over the window's 6 W unknowns: the data blocks by track_restated.jacobian, the pairs by smooth_restated.between_jacobian,
                 of the anchor pair only the J_b half
    LM           smooth_restated.smooth_lm over the window (the same loop, dict, margin and slack), rows = 8 detections + 6 pairs
    driver       Live: carries the window, the anchor and the starts from push to push as include/aar.h states them
"""
import numpy as np

import smooth_restated as sr
import track_restated as tr


class WindowProblem:
    """the problem of one push: frames (indices into td, oldest first) at times; anchor = (pose [6], time) or None"""

    def __init__(self, td, frames, times, sigma_rot=1.0, sigma_trans=1.0, delta=-1.0, anchor=None, smooth=True):
        self.td, self.frames, self.F = td, list(frames), len(frames)
        self.delta = -1.0 if delta is None else delta
        self.smooth = bool(smooth)
        self.fd = [td.frame(f) for f in self.frames]
        self.anchor = None if (anchor is None or not self.smooth) else np.array(anchor[0], dtype=np.float64)
        t = np.asarray(times, dtype=np.float64)
        # lam[i]: the pair that ENDS at window frame i (i = 0: the anchor pair)
        self.lam = np.zeros((self.F, 6))
        if self.smooth:
            dt = np.r_[(t[0] - anchor[1]) if self.anchor is not None else np.nan, np.diff(t)]
            with np.errstate(invalid="ignore"):
                self.lam[:, :3] = (1.0 / (sigma_rot * sigma_rot * dt))[:, None]
                self.lam[:, 3:] = (1.0 / (sigma_trans * sigma_trans * dt))[:, None]
            if self.anchor is None:
                self.lam[0] = 0.0
        self.detections = int(sum(fd["ou"].shape[0] for fd in self.fd))
        self.pairs = (self.F - 1 + (self.anchor is not None)) if self.smooth else 0
        self.rows = 8.0 * self.detections + 6.0 * self.pairs

    def costs(self, z):
        """(data cost per frame [W], cost of the pair that ends at each frame [W]) at z [W, 6]"""
        z = np.asarray(z, dtype=np.float64).reshape(self.F, 6)
        Ef = np.array([tr.frame_error(self.fd[i], z[i], self.delta) for i in range(self.F)])
        Pe = np.zeros(self.F)
        if self.smooth:
            for i in range(self.F):
                if i == 0 and self.anchor is None:
                    continue
                e = sr.between(self.anchor if i == 0 else z[i - 1], z[i])
                Pe[i] = float(np.sum(self.lam[i] * e * e))
        return Ef, Pe

    def cost(self, z):
        Ef, Pe = self.costs(z)
        return float(np.sum(Ef) + np.sum(Pe))

    def system(self, z):
        """(diag [W, 6, 6], off [W-1, 6, 6], rhs [6W]) at z [W, 6]"""
        z = np.asarray(z, dtype=np.float64).reshape(self.F, 6)
        F = self.F
        diag, off, rhs = np.zeros((F, 6, 6)), np.zeros((max(F - 1, 0), 6, 6)), np.zeros((F, 6))
        for i in range(F):
            J, rw = tr.jacobian(self.fd[i], z[i], self.delta)
            diag[i] = J.T @ J
            rhs[i] = -J.T @ rw
        if self.smooth:
            for i in range(F):
                if i == 0 and self.anchor is None:
                    continue
                J, e = sr.between_jacobian(self.anchor if i == 0 else z[i - 1], z[i])
                L = self.lam[i]
                Ja, Jb = J[:, :6], J[:, 6:]
                diag[i] += Jb.T @ (L[:, None] * Jb)
                rhs[i] -= Jb.T @ (L * e)
                if i > 0:
                    diag[i - 1] += Ja.T @ (L[:, None] * Ja)
                    off[i - 1] = Ja.T @ (L[:, None] * Jb)
                    rhs[i - 1] -= Ja.T @ (L * e)
        return diag, off, rhs.reshape(-1)


def push_lm(wp, z0, **lm):
    """the LM of one push from the window poses z0 [W, 6]: smooth_restated.smooth_lm's loop and dict (z, iterations, err, data, prior, exit,
    rejected, mu, margin, slack, grad0, grad)"""
    return sr.smooth_lm(wp, z0, **lm)


class Live:
    """push-by-push driver over the frames of a TrackData"""

    def __init__(self, td, lag=0, smooth=False, sigma_rot=1.0, sigma_trans=1.0, delta=-1.0, **lm):
        assert 0 <= lag <= 15 and (smooth or lag == 0)
        self.td, self.lag, self.smooth, self.sr, self.st, self.delta, self.lm = td, lag, bool(smooth), sigma_rot, sigma_trans, delta, lm
        self.reset()

    def reset(self):
        self.n = 0
        self.win = []          # [frame of td, time, pose] oldest first
        self.anchor = None     # (pose, time)

    def push(self, f, time, pose_init=None):
        """returns smooth_lm's dict plus frame_index, window_frames, pose, lagged_pose (None until the window is full), problem"""
        if pose_init is None:
            assert self.win, "the first push needs a pose_init"
            start = self.win[-1][2].copy()
        else:
            start = np.array(pose_init, dtype=np.float64)
        assert not self.win or time > self.win[-1][1]
        if len(self.win) == self.lag + 1:
            _, ta, za = self.win.pop(0)
            self.anchor = (za, ta)
        self.win.append([f, float(time), start])
        wp = WindowProblem(self.td, [w[0] for w in self.win], [w[1] for w in self.win], self.sr, self.st, self.delta,
                           anchor=self.anchor, smooth=self.smooth)
        r = push_lm(wp, np.stack([w[2] for w in self.win]), **self.lm)
        for w, z in zip(self.win, r["z"]):
            w[2] = np.array(z)
        full = len(self.win) == self.lag + 1
        r.update(frame_index=self.n, window_frames=len(self.win), pose=self.win[-1][2].copy(),
                 lagged_pose=self.win[0][2].copy() if full else None, problem=wp)
        self.n += 1
        return r

    def window(self):
        return np.stack([w[2] for w in self.win]), (None if self.anchor is None else self.anchor[0])
