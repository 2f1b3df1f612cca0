"""float64 restatement of the selected inverse behind aar_track_smooth_covariance2 under the constant-velocity prior --
TEST INFRASTRUCTURE ONLY.

The supernode cyclic reduction of csrc/smooth_cv_kernels.hip restated in numpy (frames paired into supernodes (2k, 2k + 1) of 12x12 blocks, an
identity block for the padded frame of an odd F; what each eliminated supernode keeps: Dinv, Ls, its own U; the root pivot in Dw[0]) and the
downward pass over the elimination tree that turns these into S[k] = Sigma_kk and R[k] = Sigma_{k,k+1} on the supernodes, then the 6x6
blocks.  Independent of the device code: the yardstick of its tests is numpy.linalg.inv of smooth_cv_restated.dense.

    pack         D[k] = [[H_2k,2k  H_2k,2k+1], [.^T  H_2k+1,2k+1]],  U[k] = [[H_2k,2k+2  0], [H_2k+1,2k+2  H_2k+1,2k+3]]
    eliminate    smooth_covariance_restated.eliminate on 12x12 blocks
    root         S[0] = Dw[0]^-1; a pivot of its elimination that is not above ROOT_TOL * max diag of the live rows of supernode 0 of H (the
                 diagonals of H_00 and H_11, without the padded identity) counts as non-positive
    downward     strides from the top one down to 1, supernode i an odd multiple of s, p = i - s, q = i + s:
                     G_p = Dinv[i] Ls[i]^T,  G_q = Dinv[i] U[i]
                     S_ip = -(G_p S[p] + G_q R[p]^T),  S_iq = -(G_p R[p] + G_q S[q]),  S[i] = Dinv[i] - S_ip G_p^T - S_iq G_q^T
                     R[i] = S_iq, R[p] = S_ip^T;   without q (q >= K) its terms are absent
    unpack       frame_cov[2k], frame_cov[2k+1] = the diagonal 6x6 blocks of S[k];  lag_cov[2k] = S[k][0:6, 6:12],
                 lag_cov[2k+1] = R[k][6:12, 0:6];  lag2_cov[2k] = R[k][0:6, 0:6],  lag2_cov[2k+1] = R[k][6:12, 6:12]
"""
import numpy as np

from smooth_covariance_restated import ROOT_TOL, NotPositive, _inv_spd


def pack(diag, off, off2):
    """(D [K, 12, 12], U [K, 12, 12]) of the supernodes, K = ceil(F / 2)"""
    F = diag.shape[0]
    K = (F + 1) // 2
    D, U = np.zeros((K, 12, 12)), np.zeros((K, 12, 12))
    for k in range(K):
        a, b = 2 * k, 2 * k + 1
        D[k, :6, :6] = diag[a]
        if b < F:
            D[k, 6:, 6:] = diag[b]
            D[k, :6, 6:] = off[a]
            D[k, 6:, :6] = off[a].T
        else:
            D[k, 6:, 6:] = np.eye(6)
        if a + 2 < F:
            U[k, :6, :6] = off2[a]
            U[k, 6:, :6] = off[b]
        if b + 2 < F:
            U[k, 6:, 6:] = off2[b]
    return D, U


def eliminate(D, U):
    """the reduction at mu = 0 on the supernodes: (Dw, Uw, Dinv, Ls) as the device leaves them, [K, 12, 12] each"""
    K = D.shape[0]
    Dw, Uw = np.array(D, dtype=np.float64), np.array(U, dtype=np.float64)
    Dinv, Ls = np.zeros_like(Dw), np.zeros_like(Dw)
    s = 1
    while s < K:
        for j in range(0, K, 2 * s):
            Dj = Dw[j].copy()
            if j + s < K:
                r = j + s
                inv = _inv_spd(Dw[r])
                Uj = Uw[j].copy()
                Dinv[r], Ls[r] = inv, Uj
                T = Uj @ inv
                Dj -= T @ Uj.T
                if r + s < K:
                    Uw[j] = -T @ Uw[r]
            if j - s >= 0:
                q = j - s
                T = Uw[q].T @ _inv_spd(Dw[q])
                Dj -= T @ Uw[q]
            Dw[j] = 0.5 * (Dj + Dj.T)
        s *= 2
    return Dw, Uw, Dinv, Ls


def root_inverse(Dw0, top, live):
    """Dw0^-1 under the root rule: the pivots of the elimination of the first `live` rows must exceed ROOT_TOL * top"""
    m = Dw0.copy()
    for k in range(12):
        bar = ROOT_TOL * top if k < live else 0.0
        if not m[k, k] > bar:
            raise NotPositive("root pivot %d = %g" % (k, m[k, k]))
        m[k + 1:, k + 1:] -= np.outer(m[k + 1:, k], m[k, k + 1:]) / m[k, k]
    S0 = _inv_spd(Dw0)
    return 0.5 * (S0 + S0.T)


def supernode_inverse(D, U, top, live):
    """(S [K, 12, 12] = Sigma_kk, R [K, 12, 12] with R[k] = Sigma_{k,k+1} for k < K - 1) of the block-tridiagonal supernode matrix"""
    K = D.shape[0]
    Dw, Uw, Dinv, Ls = eliminate(D, U)
    S, R = np.zeros((K, 12, 12)), np.zeros((K, 12, 12))
    S[0] = root_inverse(Dw[0], top, live)
    s = 1
    while 2 * s < K:
        s *= 2
    while s >= 1 and K > 1:
        Rn = np.zeros_like(R)           # (the device's ping-pong: a level reads what the level before wrote and rewrites every live R)
        for i in range(s, K, 2 * s):
            p, q = i - s, i + s
            Gp = Dinv[i] @ Ls[i].T
            if q < K:
                Gq = Dinv[i] @ Uw[i]
                Sip = -(Gp @ S[p] + Gq @ R[p].T)
                Siq = -(Gp @ R[p] + Gq @ S[q])
                Si = Dinv[i] - Sip @ Gp.T - Siq @ Gq.T
                Rn[i] = Siq
            else:
                Sip = -(Gp @ S[p])
                Si = Dinv[i] - Sip @ Gp.T
            S[i] = 0.5 * (Si + Si.T)
            Rn[p] = Sip.T
        R = Rn
        s //= 2
    return S, R


def unpack(S, R, F):
    """(frame_cov [F, 6, 6], lag_cov [F-1, 6, 6], lag2_cov [F-2, 6, 6]) from the supernode blocks; the padded frame is never read out"""
    fc, lc, l2 = np.zeros((F, 6, 6)), np.zeros((max(F - 1, 0), 6, 6)), np.zeros((max(F - 2, 0), 6, 6))
    for f in range(F):
        k, o = f // 2, 6 * (f % 2)
        fc[f] = S[k][o:o + 6, o:o + 6]
        if f + 1 < F:
            lc[f] = R[k][6:, :6] if o else S[k][:6, 6:]
        if f + 2 < F:
            l2[f] = R[k][o:o + 6, o:o + 6]
    return fc, lc, l2


def selected_inverse(diag, off, off2):
    """(frame_cov, lag_cov, lag2_cov) of the block-pentadiagonal H; raises NotPositive on a bad pivot"""
    F = diag.shape[0]
    if F == 0:
        z = np.zeros((0, 6, 6))
        return z, z.copy(), z.copy()
    D, U = pack(diag, off, off2)
    top = float(np.max(np.einsum("fii->fi", diag[:2])))
    S, R = supernode_inverse(D, U, top, 12 if F > 1 else 6)
    return unpack(S, R, F)


def selected_blocks(M, F):
    """the diagonal, lag-one and lag-two 6x6 blocks of a dense [6F, 6F] matrix"""
    blk = lambda a, b: M[6 * a:6 * a + 6, 6 * b:6 * b + 6]
    z = np.zeros((0, 6, 6))
    S = np.stack([blk(f, f) for f in range(F)]) if F else z
    R = np.stack([blk(f, f + 1) for f in range(F - 1)]) if F > 1 else z.copy()
    R2 = np.stack([blk(f, f + 2) for f in range(F - 2)]) if F > 2 else z.copy()
    return S, R, R2


def block_row_residual(diag, off, off2, S, R, R2):
    """The block-row identity sum_j H_fj Sigma_jf = I for every frame f, from the selected blocks alone (H_fj is zero beyond |f - j| = 2 and
    every Sigma_jf inside that band is a selected block), normalised by sum_j |H_fj|_2 |Sigma_jf|_2.  Returns the largest ratio (Frobenius
    norm of the defect on top)."""
    F = diag.shape[0]
    n2 = lambda a: np.linalg.norm(a, 2)
    worst = 0.0
    for f in range(F):
        terms = [(diag[f], S[f])]
        if f >= 1:
            terms.append((off[f - 1].T, R[f - 1]))
        if f >= 2:
            terms.append((off2[f - 2].T, R2[f - 2]))
        if f + 1 < F:
            terms.append((off[f], R[f].T))
        if f + 2 < F:
            terms.append((off2[f], R2[f].T))
        acc = -np.eye(6)
        den = 0.0
        for h, sg in terms:
            acc = acc + h @ sg
            den += n2(h) * n2(sg)
        worst = max(worst, np.linalg.norm(acc) / den)
    return float(worst)
