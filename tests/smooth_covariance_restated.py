"""float64 restatement of the selected inverse behind aar_track_smooth_covariance -- TEST INFRASTRUCTURE ONLY.

The block cyclic reduction of csrc/smooth_kernels.hip restated in numpy (what each eliminated node keeps: Dinv, Ls, its own U; the root pivot
in Dw[0]) and the downward pass over the elimination tree that turns these into the diagonal blocks S[f] = (H^-1)_ff and the lag-one blocks
R[f] = (H^-1)_{f,f+1}.  Independent of the device code: the yardstick of its tests is numpy.linalg.inv of smooth_restated.dense.

    eliminate    at stride s the even multiples of s eliminate their neighbours at +-s; node r eliminated by its left neighbour j keeps
                 Dinv[r] = D_r^-1 and Ls[r] = U_j (rows j, columns r); its own U_r (rows r, columns r + s) stays where it is
    root         S[0] = Dw[0]^-1.  Dw[0] is the Schur complement of H onto frame 0, formed by subtracting from H_00: it carries a rounding error of
                 the order eps |H_00|, so a pivot of its LDL^T that is not above ROOT_TOL * max diag H_00 cannot be told from zero and counts
                 as non-positive (the prior alone: the exact root is singular, the computed one is rounding noise of either sign)
    downward     strides from the top one down to 1, node i an odd multiple of s, p = i - s, q = i + s:
                     G_p = Dinv[i] Ls[i]^T,  G_q = Dinv[i] U[i]            (x_i = Dinv[i] b_i - G_p x_p - G_q x_q)
                     S_ip = -(G_p S[p] + G_q R[p]^T),  S_iq = -(G_p R[p] + G_q S[q]),  S[i] = Dinv[i] - S_ip G_p^T - S_iq G_q^T
                     R[i] = S_iq, R[p] = S_ip^T;   without q (q >= F) its terms are absent
"""
import numpy as np


ROOT_TOL = 64 * np.finfo(np.float64).eps


class NotPositive(ArithmeticError):
    """a pivot block that is not positive definite"""


def _inv_spd(a):
    try:
        np.linalg.cholesky(a)
    except np.linalg.LinAlgError as e:
        raise NotPositive(str(e))
    return np.linalg.inv(a)


def eliminate(diag, off):
    """the reduction at mu = 0: (Dw, Uw, Dinv, Ls) as the device leaves them, [F, 6, 6] each"""
    F = diag.shape[0]
    Dw = np.array(diag, dtype=np.float64)
    Uw = np.zeros((F, 6, 6))
    Uw[:F - 1] = off
    Dinv, Ls = np.zeros((F, 6, 6)), np.zeros((F, 6, 6))
    s = 1
    while s < F:
        for j in range(0, F, 2 * s):
            D = Dw[j].copy()
            if j + s < F:
                r = j + s
                inv = _inv_spd(Dw[r])
                U = Uw[j].copy()
                Dinv[r], Ls[r] = inv, U
                T = U @ inv
                D -= T @ U.T
                if r + s < F:
                    Uw[j] = -T @ Uw[r]
            if j - s >= 0:
                q = j - s
                T = Uw[q].T @ _inv_spd(Dw[q])
                D -= T @ Uw[q]
            Dw[j] = 0.5 * (D + D.T)
        s *= 2
    return Dw, Uw, Dinv, Ls


def selected_inverse(diag, off):
    """(S [F, 6, 6] = (H^-1)_ff, R [F-1, 6, 6] = (H^-1)_{f,f+1}) of the block-tridiagonal H; raises NotPositive on a bad pivot"""
    F = diag.shape[0]
    if F == 0:
        return np.zeros((0, 6, 6)), np.zeros((0, 6, 6))
    Dw, Uw, Dinv, Ls = eliminate(diag, off)
    S, R = np.zeros((F, 6, 6)), np.zeros((F, 6, 6))
    m = Dw[0].copy()
    for k in range(6):   # the pivots of the root's LDL^T
        if not m[k, k] > ROOT_TOL * np.max(np.diag(diag[0])):
            raise NotPositive("root pivot %d = %g" % (k, m[k, k]))
        m[k + 1:, k + 1:] -= np.outer(m[k + 1:, k], m[k, k + 1:]) / m[k, k]
    S[0] = _inv_spd(Dw[0])
    S[0] = 0.5 * (S[0] + S[0].T)
    s = 1
    while 2 * s < F:
        s *= 2
    while s >= 1 and F > 1:
        for i in range(s, F, 2 * s):
            p, q = i - s, i + s
            Gp = Dinv[i] @ Ls[i].T
            if q < F:
                Gq = Dinv[i] @ Uw[i]
                Spq = R[p].copy()
                Sip = -(Gp @ S[p] + Gq @ Spq.T)
                Siq = -(Gp @ Spq + Gq @ S[q])
                Si = Dinv[i] - Sip @ Gp.T - Siq @ Gq.T
                R[i] = Siq
            else:
                Sip = -(Gp @ S[p])
                Si = Dinv[i] - Sip @ Gp.T
            S[i] = 0.5 * (Si + Si.T)
            R[p] = Sip.T
        s //= 2
    return S, R[:F - 1]


def selected_blocks(M, F):
    """the diagonal and lag-one blocks of a dense [6F, 6F] matrix"""
    S = np.stack([M[6 * f:6 * f + 6, 6 * f:6 * f + 6] for f in range(F)]) if F else np.zeros((0, 6, 6))
    R = np.stack([M[6 * f:6 * f + 6, 6 * f + 6:6 * f + 12] for f in range(F - 1)]) if F > 1 else np.zeros((0, 6, 6))
    return S, R


def block_row_residual(diag, off, S, R):
    """The block-row identity H Sigma = I at the positions the selected blocks determine, from the blocks alone:
         (f, f)      H_{f,f-1} Sigma_{f-1,f} + H_ff Sigma_ff + H_{f,f+1} Sigma_{f,f+1}^T = I
         (f, f+1)    H_ff Sigma_{f,f+1} + H_{f,f+1} Sigma_{f+1,f+1} = 0          for f = 0           (no H_{f,f-1} Sigma_{f-1,f+1} term)
         (f+1, f)    H_{f+1,f} Sigma_ff + H_{f+1,f+1} Sigma_{f,f+1}^T = 0        for f + 1 = F - 1   (no H_{f+1,f+2} Sigma_{f+2,f} term)
    each normalised by the sum over its terms of |H_fj|_2 |Sigma_jf|_2.  Returns the largest ratio (Frobenius norm of the defect on top)."""
    F = diag.shape[0]
    n2 = lambda a: np.linalg.norm(a, 2)
    worst = 0.0
    for f in range(F):
        acc = diag[f] @ S[f] - np.eye(6)
        den = n2(diag[f]) * n2(S[f])
        if f > 0:
            acc += off[f - 1].T @ R[f - 1]
            den += n2(off[f - 1]) * n2(R[f - 1])
        if f + 1 < F:
            acc += off[f] @ R[f].T
            den += n2(off[f]) * n2(R[f])
        worst = max(worst, np.linalg.norm(acc) / den)
    if F > 1:
        acc = diag[0] @ R[0] + off[0] @ S[1]
        worst = max(worst, np.linalg.norm(acc) / (n2(diag[0]) * n2(R[0]) + n2(off[0]) * n2(S[1])))
        g = F - 2
        acc = off[g].T @ S[g] + diag[g + 1] @ R[g].T
        worst = max(worst, np.linalg.norm(acc) / (n2(off[g]) * n2(S[g]) + n2(diag[g + 1]) * n2(R[g])))
    return float(worst)
