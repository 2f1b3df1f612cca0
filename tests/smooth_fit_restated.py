"""float64 restatement of the sigma fit (aar_track_smooth_fit) -- TEST INFRASTRUCTURE ONLY.

Built on tests/smooth_restated.py (SmoothProblem, dense, between_jacobian, smooth_lm: imported, not edited) with numpy.linalg.inv of the dense H;
independent of csrc/smooth_fit_kernels.hip and of the selected inverse.

    unknowns     q = sigma_px^2, s_r = sigma_rot^2, s_t = sigma_trans^2 (per unit of frame_time); the smoother runs at the effective sigmas
                 sqrt(s_r / q), sqrt(s_t / q); the Laplace posterior is N(z, q H^-1)
    E-step       per pair f (g = f + 1, D_f its time step): with J [6, 12] = d e_f / d (z_f, z_g) by complex step and
                 C = J [[S_ff, S_fg], [S_fg^T, S_gg]] J^T  (the covariance of the linearised e_f, unscaled)
                     a_r = |phi|^2 / D_f, u_r = tr(C[:3, :3]) / D_f, a_t = |e_t|^2 / D_f, u_t = tr(C[3:, 3:]) / D_f
                 U_d = sum_f tr(V_f S_ff): directly with V_f = H_ff - the prior blocks, or by tr(H H^-1) = 6 F as
                     6 F - U_r / sigma_rot_eff^2 - U_t / sigma_trans_eff^2
    M-step       s_r <- (A_r + q U_r) / (3 (F - 1)),  s_t <- (A_t + q U_t) / (3 (F - 1)),  q <- (data_cost + q U_d) / (8 N), all from the old q
    loop         smooth from the previous track, E-step, M-step; stop when the largest relative change of an estimated sigma is below rel_tol or
                 after max_iters; one more smoothing at the fitted values
"""
import numpy as np

import smooth_restated as sr


class FitProblem:
    """the sequence behind a fit: a track_restated.TrackData with its frame times and expected motions"""

    def __init__(self, td, frame_time=None, rel_motion=None):
        self.td, self.F = td, td.F
        self.frame_time, self.rel_motion = frame_time, rel_motion
        self.dt = np.ones(td.F - 1) if frame_time is None else np.diff(np.asarray(frame_time, dtype=np.float64))
        self.N = int(td.start[td.F] - td.start[0])
        self._fd = None

    def smooth_problem(self, sigma_rot, sigma_trans):
        sp = sr.SmoothProblem.__new__(sr.SmoothProblem)
        if self._fd is None:
            sp.__init__(self.td, sigma_rot, sigma_trans, frame_time=self.frame_time, rel_motion=self.rel_motion)
            self._fd, self._rows, self._rel = sp.fd, sp.rows, sp.rel
            return sp
        # (the same object without regrouping the detections of every frame again)
        F = self.F
        sp.td, sp.F, sp.delta = self.td, F, -1.0
        sp.lam = np.zeros((F - 1, 6))
        sp.lam[:, :3] = (1.0 / (sigma_rot * sigma_rot * self.dt))[:, None]
        sp.lam[:, 3:] = (1.0 / (sigma_trans * sigma_trans * self.dt))[:, None]
        sp.rel, sp.fd, sp.rows = self._rel, self._fd, self._rows
        return sp


def estep(fp, z, sigma_rot, sigma_trans):
    """one E-step at the track z [F, 6] and the effective sigmas.  Returns a dict: terms [F-1, 4], sums [4], data_cost, U_d_direct,
    U_d_trace, H (dense)"""
    F = fp.F
    sp = fp.smooth_problem(sigma_rot, sigma_trans)
    z = np.asarray(z, dtype=np.float64).reshape(F, 6)
    diag, off, _ = sp.system(z)
    H = sr.dense(diag, off)
    Hi = np.linalg.inv(H)
    Hi = 0.5 * (Hi + Hi.T)
    terms = np.zeros((F - 1, 4))
    prior = np.zeros((F, 6, 6))
    for f in range(F - 1):
        J, e = sr.between_jacobian(z[f], z[f + 1], sp._rel(f))
        C = J @ Hi[6 * f:6 * f + 12, 6 * f:6 * f + 12] @ J.T
        terms[f] = [e[:3] @ e[:3], np.trace(C[:3, :3]), e[3:] @ e[3:], np.trace(C[3:, 3:])]
        terms[f] /= fp.dt[f]
        L = sp.lam[f]
        prior[f] += J[:, :6].T @ (L[:, None] * J[:, :6])
        prior[f + 1] += J[:, 6:].T @ (L[:, None] * J[:, 6:])
    sums = terms.sum(axis=0)
    direct = float(sum(np.trace((diag[f] - prior[f]) @ Hi[6 * f:6 * f + 6, 6 * f:6 * f + 6]) for f in range(F)))
    trace = float(6.0 * F - sums[1] / (sigma_rot * sigma_rot) - sums[3] / (sigma_trans * sigma_trans))
    Ef, _ = sp.costs(z)
    return dict(terms=terms, sums=sums, data_cost=float(np.sum(Ef)), U_d_direct=direct, U_d_trace=trace, H=H)


def mstep(sums, data_cost, U_d, q, s_r, s_t, F, N, estimate=(1, 1, 1)):
    """(q, s_r, s_t) after one M-step from the old values; estimate = (px, rot, trans) flags"""
    n_r = (sums[0] + q * sums[1]) / (3.0 * (F - 1)) if estimate[1] else s_r
    n_t = (sums[2] + q * sums[3]) / (3.0 * (F - 1)) if estimate[2] else s_t
    n_q = (data_cost + q * U_d) / (8.0 * N) if estimate[0] else q
    return n_q, n_r, n_t


def fit(fp, z0, sigma_rot, sigma_trans, max_iters=50, rel_tol=1e-3, estimate=(1, 1, 1), final=True):
    """the loop from the track z0 and the effective start values.  Returns a dict: path [iterations + 1, 3] = (sigma_px, sigma_rot,
    sigma_trans), iterations, stop_code, lm_steps, z (the track at the fitted values), sigma_px, sigma_rot, sigma_trans, sigma_rot_eff,
    sigma_trans_eff, last_rel_change, sums, U_d, data_cost, margin (the smallest decision margin of the smoothing runs)"""
    F, N = fp.F, fp.N
    q, s_r, s_t = 1.0, sigma_rot * sigma_rot, sigma_trans * sigma_trans
    er, et = sigma_rot, sigma_trans
    z = np.array(z0, dtype=np.float64).reshape(F, 6)
    path = [(1.0, sigma_rot, sigma_trans)]
    lm_steps, stop, change, margin = 0, 2, 0.0, np.inf
    e = None
    for it in range(max_iters):
        r = sr.smooth_lm(fp.smooth_problem(er, et), z)
        z, lm_steps, margin = r["z"], lm_steps + r["iterations"], min(margin, r["margin"])
        e = estep(fp, z, er, et)
        new = mstep(e["sums"], e["data_cost"], e["U_d_trace"], q, s_r, s_t, F, N, estimate)
        if not all(v > 0 and np.isfinite(v) for v in new):
            raise ArithmeticError("M-step: %r" % (new,))
        change = max(abs(np.sqrt(a) - np.sqrt(b)) / np.sqrt(b) for a, b in zip(new, (q, s_r, s_t)))
        q, s_r, s_t = new
        er, et = np.sqrt(s_r / q), np.sqrt(s_t / q)
        path.append((np.sqrt(q), np.sqrt(s_r), np.sqrt(s_t)))
        if change < rel_tol:
            stop = 1
            break
    if final:
        r = sr.smooth_lm(fp.smooth_problem(er, et), z)
        z, lm_steps, margin = r["z"], lm_steps + r["iterations"], min(margin, r["margin"])
    return dict(path=np.array(path), iterations=len(path) - 1, stop_code=stop, lm_steps=lm_steps, z=z, sigma_px=np.sqrt(q), sigma_rot=np.sqrt(s_r),
                sigma_trans=np.sqrt(s_t), sigma_rot_eff=er, sigma_trans_eff=et, last_rel_change=change, sums=e["sums"], U_d=e["U_d_trace"],
                data_cost=e["data_cost"], margin=margin)
