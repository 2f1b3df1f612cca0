"""float64 restatement of the constant-velocity smoothed track's pose and covariance at any time (aar_track_smooth_query2, DESIGN.md section
34) -- TEST INFRASTRUCTURE ONLY.

Built on tests/smooth_cv_restated.py (cv_term_jacobian by complex step), tests/smooth_restated.py (between_jacobian, so3_log) and
tests/smooth_query_restated.py (locate, times_of), none of them edited, and independent of csrc/smooth_cv_query_kernels.hip.  The answer at a
time t is what ONE Gauss-Newton step of the constant-velocity smoother reports for a frame m without detections inserted at t, linearised at
the track with m at a start pose:

    start_pose      inside a gap: the geodesic pose; after the end R_{F-1} Exp(r psi), t_{F-1} + r (t_{F-1} - t_{F-2}); before the start the
                    mirror image; F = 1: z_0
    changed_terms   (removed, added): lists of (frames, times, sigmas) with 'm' for the inserted frame -- pair 0 has two frames, a term three
    model_terms     the term list section 31's model gives for a list of frame times (what changed_terms is tested against)
    local_form      the block algebra the kernel does: P = Sigma_NN over the up to four neighbours, K = P^-1 - F_old, A, B, C of K + F_new,
                    cov = (C - B^T A^-1 B)^-1, delta_m = cov (d_m - B^T A^-1 d_N) with d = g' - g = the changed terms' right-hand sides
    gauss_markov_lag3   (H^-1)_{f,f+3} from the supernode blocks S, R of the selected inverse
"""
import numpy as np

import smooth_cv_restated as scv
import smooth_query_restated as sqr
import smooth_restated as sr
import track_restated as tr

times_of = sqr.times_of
locate = sqr.locate


def start_pose(z, times, t):
    """z_m^0 [6] of a query at t (not a frame time)"""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 6)
    F = len(times)
    a, kind = locate(times, t)
    assert kind != "on"
    if kind == "inside":
        return sr.geodesic(z[a], z[a + 1], (t - times[a]) / (times[a + 1] - times[a]))
    if F == 1:
        return np.array(z[0])
    if kind == "after":
        r = (t - times[F - 1]) / (times[F - 1] - times[F - 2])
        Rp, Rc = tr.rodrigues(z[F - 2][:3]), tr.rodrigues(z[F - 1][:3])
        psi = sr.so3_log(Rp.T @ Rc)
        return np.concatenate([sr.so3_log(Rc @ tr.rodrigues(r * psi)), z[F - 1][3:] + r * (z[F - 1][3:] - z[F - 2][3:])])
    r = (times[0] - t) / (times[1] - times[0])
    R0, R1 = tr.rodrigues(z[0][:3]), tr.rodrigues(z[1][:3])
    psi = sr.so3_log(R0.T @ R1)
    return np.concatenate([sr.so3_log(R0 @ tr.rodrigues(-r * psi)), z[0][3:] - r * (z[1][3:] - z[0][3:])])


def model_terms(n):
    """section 31's terms on n frames, as tuples of positions: pair 0 on (0, 1), term f on (f - 1, f, f + 1)"""
    return ([(0, 1)] if n > 1 else []) + [(f - 1, f, f + 1) for f in range(1, n - 1)]


def changed_terms(F, times, t):
    """(removed, added, neighbours): tuples of frames with 'm' for the inserted frame; neighbours ascending"""
    a, kind = locate(times, t)
    assert kind != "on"
    rem, add = [], []
    if kind == "inside":
        b = a + 1
        if a >= 1:
            rem.append((a - 1, a, b))
            add.append((a - 1, a, "m"))
        if b <= F - 2:
            rem.append((a, b, b + 1))
            add.append(("m", b, b + 1))
        if a == 0:
            rem.append((0, 1))
            add.append((0, "m"))
        add.append((a, "m", b))
        nb = [f for f in (a - 1, a, b, b + 1) if 0 <= f < F]
    elif kind == "after":
        if F >= 2:
            add.append((F - 2, F - 1, "m"))
            nb = [F - 2, F - 1]
        else:
            add.append((0, "m"))
            nb = [0]
    else:
        if F >= 2:
            rem.append((0, 1))
            add += [("m", 0), ("m", 0, 1)]
            nb = [0, 1]
        else:
            add.append(("m", 0))
            nb = [0]
    return rem, add, nb


def _term(frames, z, times, zm, t, sig):
    """(J [6, 6 n], e [6], L [6]) of one term on the given frames ('m' = the inserted frame)"""
    sigma_rot, sigma_trans, sigma_rot0, sigma_trans0 = sig
    zz = [zm if f == "m" else z[f] for f in frames]
    tt = [t if f == "m" else times[f] for f in frames]
    if len(frames) == 2:
        J, e = sr.between_jacobian(zz[0], zz[1])
        D = tt[1] - tt[0]
        srr, stt = sigma_rot0, sigma_trans0
    else:
        D = tt[2] - tt[1]
        J, e = scv.cv_term_jacobian(zz[0], zz[1], zz[2], D / (tt[1] - tt[0]))
        srr, stt = sigma_rot, sigma_trans
    return J, e, np.r_[np.full(3, 1.0 / (srr * srr * D)), np.full(3, 1.0 / (stt * stt * D))]


def local_system(z, times, t, sig):
    """(neighbours, F_old [6n, 6n], F_new [6n+6, 6n+6], d [6n+6]) -- the inserted frame last; d = g' - g on (N, m)"""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 6)
    F = len(times)
    rem, add, nb = changed_terms(F, times, t)
    zm = start_pose(z, times, t)
    n = len(nb)
    slot = {f: k for k, f in enumerate(nb)}
    slot["m"] = n
    Fo, Fn, d = np.zeros((6 * n + 6, 6 * n + 6)), np.zeros((6 * n + 6, 6 * n + 6)), np.zeros(6 * n + 6)
    for terms, M, sg in ((rem, Fo, 1.0), (add, Fn, -1.0)):
        for frames in terms:
            J, e, L = _term(frames, z, times, zm, t, sig)
            idx = np.concatenate([np.arange(6 * slot[f], 6 * slot[f] + 6) for f in frames])
            M[np.ix_(idx, idx)] += J.T @ (L[:, None] * J)
            d[idx] += sg * (J.T @ (L * e))       # rhs = -J^T L e: the added terms enter g', the removed ones leave it
    return nb, Fo[:6 * n, :6 * n], Fn, d


def local_form(z, times, P, t, sig, form="plain"):
    """(cov [6, 6], delta_m [6]) from P = Sigma_NN [6n, 6n] of the original problem.  form 'plain': A = P^-1 - F_old + F_new;
    'ipd': A^-1 = (I + P D)^-1 P with D = F_new_NN - F_old (no inverse of P)"""
    nb, Fo, Fn, d = local_system(z, times, t, sig)
    n = 6 * len(nb)
    B, C = Fn[:n, n:], Fn[n:, n:]
    if form == "plain":
        A = np.linalg.inv(0.5 * (P + P.T)) - Fo + Fn[:n, :n]
        AiB, Aid = np.linalg.solve(A, B), np.linalg.solve(A, d[:n])
    else:
        D = Fn[:n, :n] - Fo
        G = np.eye(n) + P @ D
        AiB, Aid = np.linalg.solve(G, P @ B), np.linalg.solve(G, P @ d[:n])
    T = C - B.T @ AiB
    cov = np.linalg.inv(0.5 * (T + T.T))
    return cov, cov @ (d[n:] - B.T @ Aid)


def neighbour_cov(Hinv, nb):
    idx = np.concatenate([np.arange(6 * f, 6 * f + 6) for f in nb])
    return Hinv[np.ix_(idx, idx)]


def query(z, times, Hinv, t, sig, form="plain"):
    """(pose [6], cov [6, 6], segment, delta_m [6]) as aar_track_smooth_query2 defines them; Hinv: the dense inverse of the original system"""
    z = np.asarray(z, dtype=np.float64).reshape(-1, 6)
    a, kind = locate(times, t)
    if kind == "on":
        return np.array(z[a]), np.array(Hinv[6 * a:6 * a + 6, 6 * a:6 * a + 6]), a, np.zeros(6)
    _, _, nb = changed_terms(len(times), times, t)
    cov, dm = local_form(z, times, neighbour_cov(Hinv, nb), t, sig, form)
    return start_pose(z, times, t) + dm, cov, a, dm


def supernode_blocks(Hinv, F):
    """S [K, 12, 12], R [K - 1, 12, 12] of the selected inverse on supernodes (2k, 2k + 1); the padded frame of an odd F: identity, uncoupled"""
    K = (F + 1) // 2
    G = np.eye(12 * K)
    G[:6 * F, :6 * F] = Hinv
    S = np.stack([G[12 * k:12 * k + 12, 12 * k:12 * k + 12] for k in range(K)])
    R = np.stack([G[12 * k:12 * k + 12, 12 * k + 12:12 * k + 24] for k in range(K - 1)]) if K > 1 else np.zeros((0, 12, 12))
    return S, R


def gauss_markov_lag3(S, R, F):
    """l3 [F - 3, 6, 6], l3[f] = (H^-1)_{f,f+3}: even f = 2k copied from R[k]; odd f = 2k - 1 by Sigma_{k-1,k+1} = Sigma_{k-1,k} Sigma_kk^-1
    Sigma_{k,k+1} of a block-tridiagonal H"""
    out = np.zeros((max(F - 3, 0), 6, 6))
    for f in range(F - 3):
        if f % 2 == 0:
            out[f] = R[f // 2][0:6, 6:12]
        else:
            k = (f + 1) // 2
            out[f] = (R[k - 1] @ np.linalg.inv(S[k]) @ R[k])[6:12, 0:6]
    return out
