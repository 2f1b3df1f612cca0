"""float64 numpy restatement of the relative pose priors (include/aar.h, aar_pair_prior) -- TEST INFRASTRUCTURE ONLY.

A pair is (kind, a, b, x6_rel, info): two cameras or two markers by problem index, x6_rel the (rvec, t) of the prior for T_a^-1 T_b, info the
6x6 information matrix L.  With (R, t) the entities' poses in x_full (a root is the identity):

    R_ab = R_a^T R_b,  t_ab = R_a^T (t_b - t_a),  phi = log(R_rel^T R_ab)^v,  e = [phi ; t_ab - t_rel],  cost = e^T L e

and over the z entries (w_a, t_a), (w_b, t_b), with R(w + dw) = Exp(J_l(w) dw) R:

    J_a = [ -J_r(phi)^-1 R_b^T J_l(w_a)   0 ;  R_a^T [t_b - t_a]x J_l(w_a)   -R_a^T ]      J_b = [ J_r(phi)^-1 R_b^T J_l(w_b)   0 ;  0   R_a^T ]

Nothing here calls the library; the SO(3) pieces are those of tests/reduced_system.py (the pose priors' restatement)."""
import numpy as np

from reduced_system import hat, jl, jr_inv, rodrigues, slot_col, so3_log


def relative_pose(xa, xb):
    """(rvec, t) of T_a^-1 T_b"""
    Ra, Rb = rodrigues(xa[:3]), rodrigues(xb[:3])
    return np.r_[so3_log(Ra.T @ Rb), Ra.T @ (xb[3:] - xa[3:])]


def pair_e(xa, xb, xrel):
    Ra, Rb = rodrigues(xa[:3]), rodrigues(xb[:3])
    Rab = Ra.T @ Rb
    return np.r_[so3_log(rodrigues(xrel[:3]).T @ Rab), Ra.T @ (xb[3:] - xa[3:]) - xrel[3:]]


def pair_J(xa, xb, xrel):
    """analytic (J_a, J_b), 6x6 each"""
    Ra, Rb = rodrigues(xa[:3]), rodrigues(xb[:3])
    phi = pair_e(xa, xb, xrel)[:3]
    Ji = jr_inv(phi)
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    Ja[:3, :3] = -Ji @ Rb.T @ jl(xa[:3])
    Jb[:3, :3] = Ji @ Rb.T @ jl(xb[:3])
    Ja[3:, :3] = Ra.T @ hat(xb[3:] - xa[3:]) @ jl(xa[:3])
    Ja[3:, 3:] = -Ra.T
    Jb[3:, 3:] = Ra.T
    return Ja, Jb


def pair_J_numeric(xa, xb, xrel, h=1e-6):
    """central differences of e over (w_a, t_a) and (w_b, t_b)"""
    Ja, Jb = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Ja[:, k] = (pair_e(xa + d, xb, xrel) - pair_e(xa - d, xb, xrel)) / (2 * h)
        Jb[:, k] = (pair_e(xa, xb + d, xrel) - pair_e(xa, xb - d, xrel)) / (2 * h)
    return Ja, Jb


def is_root(ds, kind, idx):
    return idx == (ds.root_cam if kind == "camera" else ds.root_marker)


def pose_of(ds, x, kind, idx):
    """the entity's (rvec, t) in x_full; a root is the identity"""
    if is_root(ds, kind, idx):
        return np.zeros(6)
    c = slot_col(ds, kind, idx)
    return np.array(x[c:c + 6], dtype=np.float64)


def pair_residuals(ds, x, pairs):
    return np.array([pair_e(pose_of(ds, x, k, a), pose_of(ds, x, k, b), np.asarray(xr, float)) for k, a, b, xr, _ in pairs]).reshape(len(pairs), 6)


def pair_terms(ds, x, pairs, P, fixed=()):
    """dense J^T L J (P x P), -J^T L e, sum e^T L e of the pairs at x.  fixed: (kind, index) of caller-fixed entities; a fixed end (those and
    the roots) is a constant of its term: no rows, no columns.  Also returns the list of touched (row column, col column) 6x6 blocks."""
    H = np.zeros((P, P))
    B = np.zeros(P)
    cost = 0.0
    touched = []
    fixed = set(fixed)
    for kind, a, b, xrel, info in pairs:
        xa, xb, xrel = pose_of(ds, x, kind, a), pose_of(ds, x, kind, b), np.asarray(xrel, float)
        info = np.asarray(info, float).reshape(6, 6)
        e = pair_e(xa, xb, xrel)
        Ja, Jb = pair_J(xa, xb, xrel)
        cost += e @ info @ e
        ends = [(i, J) for i, J in ((a, Ja), (b, Jb)) if not is_root(ds, kind, i) and (kind, i) not in fixed]
        for i, Ji_ in ends:
            ci = slot_col(ds, kind, i)
            B[ci:ci + 6] -= Ji_.T @ info @ e
            for j, Jj in ends:
                cj = slot_col(ds, kind, j)
                H[ci:ci + 6, cj:cj + 6] += Ji_.T @ info @ Jj
                touched.append((ci, cj))
    return H, B, cost, touched
