"""float64 restatement of the sigma fit under the constant-velocity prior (aar_track_smooth_fit2) -- TEST INFRASTRUCTURE
ONLY.

Built on tests/smooth_cv_restated.py (SmoothCvProblem, dense, cv_term_jacobian, smooth_lm) and tests/smooth_fit_restated.py / smooth_restated.py
(between_jacobian), all imported and not edited, with numpy.linalg.inv of the dense H; independent of csrc/smooth_cv_fit_kernels.hip, of the
selected inverse and of the block structure of the term's Jacobian.

    unknowns     q = sigma_px^2, s_r = sigma_rot^2, s_t = sigma_trans^2 of the terms 1 .. F-2; pair 0's sigmas are physical and held: every
                 smoothing runs at sqrt(s_r / q), sqrt(s_t / q), sigma_rot0 / sqrt(q), sigma_trans0 / sqrt(q)
    E-step       term f (1 <= f <= F-2, D_f its time step): J [6, 18] = d e_f / d (z_{f-1}, z_f, z_{f+1}) by complex step,
                 C = J Sigma J^T with Sigma the 18 x 18 block of H^-1 over the three frames
                     a_r = |phi|^2 / D_f, u_r = tr(C[:3, :3]) / D_f, a_t = |e_t|^2 / D_f, u_t = tr(C[3:, 3:]) / D_f
                 entry 0: pair 0 the same way with smooth_restated.between_jacobian [6, 12] and D_0
                 sums over the entries 1 .. F-2 only; u_0 = u_r[0] / sigma_rot0_eff^2 + u_t[0] / sigma_trans0_eff^2
                 U_d = sum_f tr(V_f S_ff): directly with V_f = H_ff - the prior blocks, or by tr(H H^-1) = 6 F as
                     6 F - U_r / sigma_rot_eff^2 - U_t / sigma_trans_eff^2 - u_0
    M-step       s_r <- (A_r + q U_r) / (3 (F - 2)),  s_t <- (A_t + q U_t) / (3 (F - 2)),  q <- (data_cost + q U_d) / (8 N), all from the old q
    loop         smooth_fit_restated.fit's: smooth from the previous track, E-step, M-step; stop when the largest relative change of an estimated
                 sigma is below rel_tol or after max_iters; one more smoothing at the fitted values
"""
import copy

import numpy as np

import smooth_cv_restated as cvr
import smooth_fit_restated as fr
import smooth_restated as sr


class CvFitProblem(fr.FitProblem):
    """the sequence behind a fit: smooth_fit_restated.FitProblem's fields (td, F, frame_time, dt, N) with pair 0's physical sigmas"""

    def __init__(self, td, sigma_rot0, sigma_trans0, frame_time=None):
        fr.FitProblem.__init__(self, td, frame_time)
        self.sigma_rot0, self.sigma_trans0 = sigma_rot0, sigma_trans0
        self._first = None

    def smooth_problem(self, sigma_rot, sigma_trans, sigma_rot0, sigma_trans0):
        """SmoothCvProblem at the four effective sigmas"""
        if self._first is None:
            self._first = cvr.SmoothCvProblem(self.td, sigma_rot, sigma_trans, sigma_rot0, sigma_trans0, frame_time=self.frame_time)
            return self._first
        # (the same object without regrouping the detections of every frame again)
        sp = copy.copy(self._first)
        sp.lam = np.zeros((self.F - 1, 6))
        sp.lam[:, :3] = (1.0 / (sigma_rot * sigma_rot * self.dt))[:, None]
        sp.lam[:, 3:] = (1.0 / (sigma_trans * sigma_trans * self.dt))[:, None]
        sp.lam[0, :3] = 1.0 / (sigma_rot0 * sigma_rot0 * self.dt[0])
        sp.lam[0, 3:] = 1.0 / (sigma_trans0 * sigma_trans0 * self.dt[0])
        return sp


def estep(fp, z, sigma_rot, sigma_trans, sigma_rot0, sigma_trans0):
    """one E-step at the track z [F, 6] and the effective sigmas.  Returns a dict: terms [F-1, 4] (entry 0: pair 0), sums [4] over the entries
    1 .. F-2, u_0, pair0_cost, data_cost, U_d_direct, U_d_trace, H (dense)"""
    F = fp.F
    sp = fp.smooth_problem(sigma_rot, sigma_trans, sigma_rot0, sigma_trans0)
    z = np.asarray(z, dtype=np.float64).reshape(F, 6)
    diag, off, off2, _ = sp.system(z)
    H = cvr.dense(diag, off, off2)
    Hi = np.linalg.inv(H)
    Hi = 0.5 * (Hi + Hi.T)
    terms = np.zeros((F - 1, 4))
    prior = np.zeros((F, 6, 6))
    for f in range(F - 1):
        if f == 0:
            J, e = sr.between_jacobian(z[0], z[1])
            first, n = 0, 2
        else:
            J, e = cvr.cv_term_jacobian(z[f - 1], z[f], z[f + 1], sp.ratio[f])
            first, n = f - 1, 3
        C = J @ Hi[6 * first:6 * (first + n), 6 * first:6 * (first + n)] @ J.T
        terms[f] = [e[:3] @ e[:3], np.trace(C[:3, :3]), e[3:] @ e[3:], np.trace(C[3:, 3:])]
        terms[f] /= fp.dt[f]
        L = sp.lam[f]
        for a in range(n):
            Ja = J[:, 6 * a:6 * a + 6]
            prior[first + a] += Ja.T @ (L[:, None] * Ja)
    sums = terms[1:].sum(axis=0)
    u_0 = float(terms[0, 1] / (sigma_rot0 * sigma_rot0) + terms[0, 3] / (sigma_trans0 * sigma_trans0))
    direct = float(sum(np.trace((diag[f] - prior[f]) @ Hi[6 * f:6 * f + 6, 6 * f:6 * f + 6]) for f in range(F)))
    trace = float(6.0 * F - sums[1] / (sigma_rot * sigma_rot) - sums[3] / (sigma_trans * sigma_trans) - u_0)
    Ef, Pe = sp.costs(z)
    return dict(terms=terms, sums=sums, u_0=u_0, pair0_cost=float(Pe[0]), data_cost=float(np.sum(Ef)), U_d_direct=direct, U_d_trace=trace, H=H)


def mstep(sums, data_cost, U_d, q, s_r, s_t, F, N, estimate=(1, 1, 1)):
    """(q, s_r, s_t) after one M-step from the old values; estimate = (px, rot, trans) flags"""
    n_r = (sums[0] + q * sums[1]) / (3.0 * (F - 2)) if estimate[1] else s_r
    n_t = (sums[2] + q * sums[3]) / (3.0 * (F - 2)) if estimate[2] else s_t
    n_q = (data_cost + q * U_d) / (8.0 * N) if estimate[0] else q
    return n_q, n_r, n_t


def fit(fp, z0, sigma_rot, sigma_trans, max_iters=50, rel_tol=1e-3, estimate=(1, 1, 1), final=True):
    """the loop from the track z0 and the effective start values (pair 0's sigmas: fp's).  Returns smooth_fit_restated.fit's dict, with u_0."""
    F, N = fp.F, fp.N
    q, s_r, s_t = 1.0, sigma_rot * sigma_rot, sigma_trans * sigma_trans
    eff = (sigma_rot, sigma_trans, fp.sigma_rot0, fp.sigma_trans0)
    z = np.array(z0, dtype=np.float64).reshape(F, 6)
    path = [(1.0, sigma_rot, sigma_trans)]
    lm_steps, stop, change, margin = 0, 2, 0.0, np.inf
    e = None
    for it in range(max_iters):
        r = cvr.smooth_lm(fp.smooth_problem(*eff), z)
        z, lm_steps, margin = r["z"], lm_steps + r["iterations"], min(margin, r["margin"])
        e = estep(fp, z, *eff)
        new = mstep(e["sums"], e["data_cost"], e["U_d_trace"], q, s_r, s_t, F, N, estimate)
        if not all(v > 0 and np.isfinite(v) for v in new):
            raise ArithmeticError("M-step: %r" % (new,))
        change = max(abs(np.sqrt(a) - np.sqrt(b)) / np.sqrt(b) for a, b in zip(new, (q, s_r, s_t)))
        q, s_r, s_t = new
        eff = (np.sqrt(s_r / q), np.sqrt(s_t / q), fp.sigma_rot0 / np.sqrt(q), fp.sigma_trans0 / np.sqrt(q))
        path.append((np.sqrt(q), np.sqrt(s_r), np.sqrt(s_t)))
        if change < rel_tol:
            stop = 1
            break
    if final:
        r = cvr.smooth_lm(fp.smooth_problem(*eff), z)
        z, lm_steps, margin = r["z"], lm_steps + r["iterations"], min(margin, r["margin"])
    return dict(path=np.array(path), iterations=len(path) - 1, stop_code=stop, lm_steps=lm_steps, z=z, sigma_px=np.sqrt(q), sigma_rot=np.sqrt(s_r),
                sigma_trans=np.sqrt(s_t), sigma_rot_eff=eff[0], sigma_trans_eff=eff[1], last_rel_change=change, sums=e["sums"], u_0=e["u_0"],
                U_d=e["U_d_trace"], data_cost=e["data_cost"], margin=margin)

