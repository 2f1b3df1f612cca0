"""float64 restatement of aar_track_smooth_relative -- TEST INFRASTRUCTURE ONLY.

The covariance between any two frames from the blocks a selected inverse holds, by the Gauss-Markov chain of a block-tridiagonal H:

    Sigma_ab = Sigma_ak Sigma_kk^-1 Sigma_kb  for a < k < b,   so   Sigma_ab = Sigma_{a,a+1} C_{a+1} ... C_{b-1},  C_k = Sigma_kk^-1 Sigma_{k,k+1}

    random walk         on frames: S [F, 6, 6] = Sigma_ff, R [F-1, 6, 6] = Sigma_{f,f+1}; lags 0 and 1 are S and R themselves
    constant velocity   on supernodes K = frames (2K, 2K + 1): S12 [Kn, 12, 12], R12 [Kn-1, 12, 12], the padded frame of an odd F an identity row
                        and column of the last supernode; lags 0 .. 3 come straight from Sigma's blocks, the rest is the 6x6 sub-block
                        (a mod 2, b mod 2) of the supernode chain from K_a to K_b

(a, b) with a > b is the transpose of (b, a).  The relative motion and its covariance:

    rel     = between(z_a, z_b) of tests/smooth_restated.py, no expected motion
    rel_cov = J_a S_aa J_a^T + J_b S_bb J_b^T + J_a S_ab J_b^T + (J_a S_ab J_b^T)^T,  J_a = [M_a 0; 0 -I],  J_b = [M_b 0; 0 I]
              M_b = J_r^-1(phi) J_r(w_b),  M_a = -J_r^-1(phi) R_b^T R_a J_r(w_a)   (closed forms; phi = rel[:3], w the rotation vectors)

Independent of csrc/smooth_relative_kernels.hip; the yardstick it is held to is numpy.linalg.inv and the complex-step Jacobian.
"""
import numpy as np

import smooth_restated as sr
import track_restated as tr


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def so3_jr(w):
    """right Jacobian of SO(3): R(w + d) ~ R(w) Exp(J_r(w) d)"""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    W = _hat(w)
    if th < 1e-4:
        a, b = 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        a, b = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) - a * W + b * (W @ W)


def so3_jr_inv(w):
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    W = _hat(w)
    c = 1.0 / 12 + th * th / 720 if th < 1e-4 else 1 / th ** 2 - (1 + np.cos(th)) / (2 * th * np.sin(th))
    return np.eye(3) + 0.5 * W + c * (W @ W)


def rel(za, zb):
    """[log(R_a^T R_b)^v ; t_b - t_a]"""
    return sr.between(np.asarray(za, dtype=np.float64), np.asarray(zb, dtype=np.float64))


def jacobians(za, zb):
    """(J_a, J_b) [6, 6] each, in closed form"""
    za, zb = np.asarray(za, dtype=np.float64), np.asarray(zb, dtype=np.float64)
    phi = rel(za, zb)[:3]
    Ra, Rb = tr.rodrigues(za[:3]), tr.rodrigues(zb[:3])
    Ji = so3_jr_inv(phi)
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    Ja[:3, :3] = -Ji @ Rb.T @ Ra @ so3_jr(za[:3])
    Jb[:3, :3] = Ji @ so3_jr(zb[:3])
    Ja[3:, 3:] = -np.eye(3)
    Jb[3:, 3:] = np.eye(3)
    return Ja, Jb


def summands(za, zb, Saa, Sbb, Sab):
    """the four summands of rel_cov"""
    Ja, Jb = jacobians(za, zb)
    X = Ja @ Sab @ Jb.T
    return Ja @ Saa @ Ja.T, Jb @ Sbb @ Jb.T, X, X.T


def rel_cov(za, zb, Saa, Sbb, Sab):
    return sum(summands(za, zb, Saa, Sbb, Sab))


def rel_cov_complex_step(za, zb, Saa, Sbb, Sab):
    """J Sigma J^T on the joint 12x12 block, J = d between / d (z_a, z_b) by the complex step"""
    J, _ = sr.between_jacobian(za, zb)
    return J @ np.block([[Saa, Sab], [Sab.T, Sbb]]) @ J.T


def block(Sigma, a, b):
    return Sigma[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def rw_blocks(Sigma, F):
    """what the tridiagonal selected inverse holds: (S [F, 6, 6], R [F-1, 6, 6])"""
    S = np.array([block(Sigma, f, f) for f in range(F)]).reshape(F, 6, 6)
    R = np.array([block(Sigma, f, f + 1) for f in range(F - 1)]).reshape(max(F - 1, 0), 6, 6)
    return S, R


def rw_cross(S, R, a, b):
    lo, hi = min(a, b), max(a, b)
    if lo == hi:
        return np.array(S[a])
    X = np.array(R[lo])
    for k in range(lo + 1, hi):
        X = X @ np.linalg.solve(S[k], R[k])
    return X.T if a > b else X


def cv_blocks(Sigma, F):
    """the supernode blocks of the pentadiagonal selected inverse: (S12 [Kn, 12, 12], R12 [Kn-1, 12, 12])"""
    Kn = (F + 1) // 2
    P = np.eye(12 * Kn)
    P[:6 * F, :6 * F] = Sigma
    S12 = np.array([P[12 * k:12 * k + 12, 12 * k:12 * k + 12] for k in range(Kn)]).reshape(Kn, 12, 12)
    R12 = np.array([P[12 * k:12 * k + 12, 12 * k + 12:12 * k + 24] for k in range(Kn - 1)]).reshape(max(Kn - 1, 0), 12, 12)
    return S12, R12


def cv_cross(S12, R12, a, b):
    lo, hi = min(a, b), max(a, b)
    ka, kb = lo // 2, hi // 2
    ro, co = 6 * (lo % 2), 6 * (hi % 2)
    if ka == kb:
        X = S12[ka][ro:ro + 6, co:co + 6]
    else:
        P = np.array(R12[ka])
        for k in range(ka + 1, kb):
            P = P @ np.linalg.solve(S12[k], R12[k])
        X = P[ro:ro + 6, co:co + 6]
    return np.array(X.T if a > b else X)


def direct_lag(model):
    """the largest lag the device answers from blocks that exist"""
    return 3 if model == "cv" else 1


def counts(pairs, model):
    """(num_direct, num_chained, max_lag) of the report"""
    lag = np.abs(np.asarray(pairs).reshape(-1, 2)[:, 0] - np.asarray(pairs).reshape(-1, 2)[:, 1])
    d = int(np.sum(lag <= direct_lag(model)))
    return d, len(lag) - d, int(lag.max()) if len(lag) else 0
