"""float64 restatement of the smoothed track's pose and covariance at any time (aar_track_smooth_query) -- TEST
INFRASTRUCTURE ONLY.

Built on tests/smooth_restated.py (between_jacobian by complex step, geodesic) and independent of csrc/smooth_query_kernels.hip.  The answer
at a time t is what the smoother reports for a frame without detections inserted at t:

    locate        the frame a with times[a] <= t < times[a + 1]; -1 before the start, F - 1 after the end
    pose          on a frame: z_a; inside a gap: geodesic(z_a, z_b, alpha); outside: the end frame's
    factor        F(z_i, z_j, D) = J^T L J [12, 12] of one between factor without rel_motion, L = diag(1 / (sigma_rot^2 D) x3, 1 / (sigma_trans^2 D) x3)
    block_form    the 6x6 block algebra the kernel does: P^-1 by a block Schur complement, K = P^-1 - F(z_a, z_b, D), the two new factors on
                  top, (a, b) eliminated by a second block Schur complement, the remaining 6x6 inverted
    plain_form    the same 18 x 18 (12 x 12 outside) information assembled densely and inverted by numpy: the form the definition states
"""
import numpy as np

import smooth_restated as sr


def times_of(F, frame_time=None):
    return np.arange(F, dtype=np.float64) if frame_time is None else np.asarray(frame_time, dtype=np.float64)


def locate(times, t):
    """(segment, kind): kind 'on' (t == times[segment]), 'inside' (the gap after segment), 'before' (segment -1), 'after' (segment F - 1)"""
    F = len(times)
    a = int(np.searchsorted(times, t, side="right")) - 1
    if a < 0:
        return -1, "before"
    if times[a] == t:
        return a, "on"
    if a == F - 1:
        return a, "after"
    return a, "inside"


def pose(z, times, t):
    a, kind = locate(times, t)
    if kind == "before":
        return np.array(z[0])
    if kind in ("on", "after"):
        return np.array(z[a])
    return sr.geodesic(z[a], z[a + 1], (t - times[a]) / (times[a + 1] - times[a]))


def factor(zi, zj, D, sigma_rot, sigma_trans):
    J, _ = sr.between_jacobian(zi, zj)
    L = np.r_[np.full(3, 1.0 / (sigma_rot * sigma_rot * D)), np.full(3, 1.0 / (sigma_trans * sigma_trans * D))]
    return J.T @ (L[:, None] * J)


def _inv(M):
    return np.linalg.inv(0.5 * (M + M.T))


def block_form(z, times, S, R, t, sigma_rot, sigma_trans):
    """the covariance block at t from S [F, 6, 6], R [F-1, 6, 6] on 6x6 blocks only"""
    a, kind = locate(times, t)
    if kind == "on":
        return np.array(S[a])
    if kind in ("before", "after"):
        e = 0 if kind == "before" else a
        D = abs(t - times[e])
        Fm = factor(z[e], z[e], D, sigma_rot, sigma_trans)
        me, ee = (slice(0, 6), slice(6, 12)) if kind == "before" else (slice(6, 12), slice(0, 6))
        M = _inv(S[e]) + Fm[ee, ee]
        return _inv(Fm[me, me] - Fm[me, ee] @ _inv(M) @ Fm[ee, me])
    b = a + 1
    D = times[b] - times[a]
    zm = pose(z, times, t)
    F0 = factor(z[a], z[b], D, sigma_rot, sigma_trans)
    F1 = factor(z[a], zm, t - times[a], sigma_rot, sigma_trans)
    F2 = factor(zm, z[b], times[b] - t, sigma_rot, sigma_trans)
    lo, hi = slice(0, 6), slice(6, 12)
    # P^-1 on blocks: X = S_b - R^T S_a^-1 R
    Ia = _inv(S[a])
    W = Ia @ R[a]
    Xi = _inv(S[b] - R[a].T @ W)
    V = W @ Xi
    Maa = Ia + V @ W.T - F0[lo, lo] + F1[lo, lo]
    Mab = -V - F0[lo, hi]
    Mbb = Xi - F0[hi, hi] + F2[hi, hi]
    Ba, Bb = F1[lo, hi], F2[hi, lo]                     # the couplings (a, m) and (b, m)
    C = F1[hi, hi] + F2[lo, lo]
    Ii = _inv(Maa)
    G = Ii @ Ba
    Z = Ii @ Mab
    Yi = _inv(Mbb - Mab.T @ Z)
    E = Bb - Mab.T @ G
    return _inv(C - Ba.T @ G - E.T @ Yi @ E)


def plain_form(z, times, S, R, t, sigma_rot, sigma_trans):
    """the definition, densely: the (m, m) block of the inverse of the 18 x 18 (12 x 12 outside the sequence) information"""
    a, kind = locate(times, t)
    if kind == "on":
        return np.array(S[a])
    if kind in ("before", "after"):
        e = 0 if kind == "before" else a
        Fm = factor(z[e], z[e], abs(t - times[e]), sigma_rot, sigma_trans)
        M = np.array(Fm)
        ee = slice(6, 12) if kind == "before" else slice(0, 6)
        M[ee, ee] += np.linalg.inv(S[e])
        Mi = np.linalg.inv(M)
        return Mi[0:6, 0:6] if kind == "before" else Mi[6:12, 6:12]
    b = a + 1
    zm = pose(z, times, t)
    P = np.block([[S[a], R[a]], [R[a].T, S[b]]])
    M = np.zeros((18, 18))
    M[:12, :12] = np.linalg.inv(P) - factor(z[a], z[b], times[b] - times[a], sigma_rot, sigma_trans)
    am = np.r_[0:6, 12:18]
    mb = np.r_[12:18, 6:12]
    M[np.ix_(am, am)] += factor(z[a], zm, t - times[a], sigma_rot, sigma_trans)
    M[np.ix_(mb, mb)] += factor(zm, z[b], times[b] - t, sigma_rot, sigma_trans)
    return np.linalg.inv(M)[12:, 12:]
