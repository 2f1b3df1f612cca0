"""Certificate of one step of the direct chain (k_frame_inv -> k_schur* -> k_ldl_* -> k_backsub) -- TEST INFRASTRUCTURE ONLY, numpy only.

The chain solves the damped reduced system of the device's own dense normal equations, so the certificate takes H, B from
Problem.eval_normal_equations (or, on the host, from the oracle) and restates only what the chain does (tests/reduced_system.py):

    A = U - sum_f W_f V_f^-1 W_f^T     b = g_s - sum_f W_f V_f^-1 g_f     A d_s = b     d_f = V_f^-1 (g_f - W_f^T d_s)

(a) reduced residual, r = b - A d_s evaluated in np.longdouble (where that is wider than float64; else the float64 evaluation's own
    n u (|A| |d_s| + |b|) joins the bar):

        |r|_2 <= gamma (E_A |d_s|_2 + E_b) + slack
        E_A   = | |U| + sum_f kappa_f |W_f| |V_f^-1| |W_f^T| |_F          kappa_f = cond_2(V_f + mu I)
        E_b   = | |g_s| + sum_f kappa_f |W_f| |V_f^-1| |g_f| |_2
        gamma = (3 n + 12 F_max + 64) 2^-53     n: reduced unknowns, F_max: the most frames any one entity is seen in
        slack = | |A| |z_s| |_2 2.3e-16         (the step comes back as a difference of two pose vectors)

    The slack: the step is read back as fl(z1 - z0) with z1 = fl(z0 + d), so component j of the returned d_s is off by at most ulp |z_j|, and row i
    of the residual by at most ulp sum_j |A_ij| |z_j|.  By Cauchy-Schwarz that is never more than |A|_F ulp |z_s|, the bound of the inexact
    solvers' certificate; at mu = max diag H, where A is close to mu I, it is smaller by about sqrt(n), and so it is used here: with the
    Frobenius product the slack was half of the bar of a seven-tile system and hid a relative error of 1e-9 in a block.

    gamma is an operation count: a block of S seen in F_max frames is a sum of 6 F_max six-term products formed twice (Y = W V^-1, then
    Y W^T), the factorisation and the two substitutions add at most 3 n rounded operations per entry.  The inverse of V_f is good to
    kappa_f u, hence the weight of every frame's share.  Nothing here is fitted to what a kernel gives.
(b) where: the same inequality block row by block row (one block per entity: 6 rows, 9 for an intrinsics entity); a failure names the
    block with the largest |r_a| / (gamma (E_A |d_s| + E_b)_a + slack_a), its entity kind and index.  By the triangle inequality the
    block bars add up to no more than the global one, so a step whose every block passes passes (a).
(c) frame part: d_f against backsub(d_s) of the same system, per frame 1e-10 of the size of the subtracted terms plus the rounding of z --
    the bar of the inexact solvers' certificate (tests/test_gpu_solve_certificates.py, certify); entries of fixed entities exactly 0.0.
(d) (a forward bound in the energy norm) is NOT stated: |d_s - A^-1 b|_A = |A^-1/2 r| <= |r| / lambda_min(A)^1/2, so the bound
    gamma kappa_2(A)^1/2 (E_A |d_s| + E_b) / lambda_min^1/2 is (a) divided by lambda_min^1/2 and loosened by kappa^1/2: every step that meets
    (a) meets it.  What a max-norm forward error hides -- a wrong small component -- shows in (b), whose bars are per block row.
"""
import numpy as np

from reduced_system import ReducedSystem, held_mask, split_indices

U53 = 2.0 ** -53
ULP = 2.3e-16                           # rounding of a difference of two pose vectors, relative to |z|
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def entity_blocks(ds, optimize=(True, True, True), intrinsics=False):
    """[(kind, index, first reduced unknown, size)] of the entity unknowns in z order: cameras and markers without their roots, then the
    intrinsics entities of all cameras"""
    oc, om, _ = optimize
    out, o = [], 0
    if oc:
        for c in range(ds.num_cams):
            if c != ds.root_cam:
                out.append(("camera", c, o, 6))
                o += 6
    if om:
        for m in range(ds.num_markers):
            if m != ds.root_marker:
                out.append(("marker", m, o, 6))
                o += 6
    if intrinsics:
        for c in range(ds.num_cams):
            out.append(("intrinsics", c, o, 9))
            o += 9
    return out


def build_system(ds, H, B, mu, optimize=(True, True, True), intrinsics=False, fixed_cams=(), fixed_markers=(), Hp=None, Bp=None):
    """the damped reduced system of H, B (the device's own carry the pose priors already; the oracle's take them as Hp, Bp)"""
    ent, frames = split_indices(ds, optimize, intrinsics)
    held = held_mask(ds, len(B), fixed_cams, fixed_markers)
    return ReducedSystem(H, B, mu, ent, frames, held=held, Hp=Hp, Bp=Bp)


class DirectCertificateError(AssertionError):
    pass


def gamma(rs):
    fmax = int(rs.frames_seen().max()) if len(rs.ent) else 0
    return (3 * len(rs.ent) + 12 * fmax + 64) * U53


def residual_bars(rs, ds_, zs, blocks):
    """(r [n] in the widest float, global bar, per-block |r_a|, per-block bars)"""
    n = len(rs.ent)
    EA, Eb = rs.abs_sums()
    g = gamma(rs)
    nd = np.linalg.norm(ds_)
    if WIDE:
        r = rs.b64.astype(np.longdouble) - rs.A64.astype(np.longdouble) @ ds_.astype(np.longdouble)
        own = np.zeros(n)
        own_glob = 0.0
    else:
        r = rs.b64 - rs.A64 @ ds_
        own = n * U53 * (np.linalg.norm(rs.A64, axis=1) * nd + np.abs(rs.b64))
        own_glob = n * U53 * (np.linalg.norm(rs.A64) * nd + np.linalg.norm(rs.b64))
    r = np.asarray(r, dtype=np.float64)
    sl = ULP * (np.abs(rs.A64) @ np.abs(zs))          # rounding of z0 + d, row by row
    bar = g * (np.linalg.norm(EA) * nd + np.linalg.norm(Eb)) + np.linalg.norm(sl) + own_glob
    rb, bb = [], []
    for kind, idx, o, sz in blocks:
        s = slice(o, o + sz)
        rb.append(np.linalg.norm(r[s]))
        bb.append(g * (np.linalg.norm(EA[s]) * nd + np.linalg.norm(Eb[s])) + np.linalg.norm(sl[s]) + np.linalg.norm(own[s]))
    return r, bar, np.array(rb), np.array(bb)


def block_resolution(rs, ds_, zs, blocks, i, j):
    """the relative error of block (i, j) of A (and of its mirror) that the bar of (a) resolves for the step ds_: bar / |(A_ij d_j, A_ji d_i)|.
    A step from a system whose block is off by more than that fails (a); a smaller error hides in the bar."""
    _, bar, _, _ = residual_bars(rs, ds_, zs, blocks)
    (oi, si), (oj, sj) = blocks[i][2:], blocks[j][2:]
    share = np.hypot(np.linalg.norm(rs.A64[oi:oi + si, oj:oj + sj] @ ds_[oj:oj + sj]), np.linalg.norm(rs.A64[oj:oj + sj, oi:oi + si] @ ds_[oi:oi + si]))
    return bar / max(share, 1e-300)


def certify_direct(rs, delta, z, blocks, what="", frame_part=True):
    """assert (a), (b), (c) for the step delta (z order) that ends at the pose vector z.  Returns dict(ratio, worst_block, frame_ratio)."""
    ds_, df = rs.split(delta)
    zs, zf = rs.split(z)
    out = dict(ratio=0.0, worst_block=None, frame_ratio=0.0)
    if rs.held_e.any() and not np.all(ds_[rs.held_e] == 0.0):
        raise DirectCertificateError((what, "a fixed entity moved", np.nonzero(rs.held_e & (ds_ != 0.0))[0][:6]))
    if len(ds_):
        if not np.all(np.isfinite(ds_)):
            raise DirectCertificateError((what, "the step is not finite"))
        r, bar, rb, bb = residual_bars(rs, ds_, zs, blocks)
        ratio = float(np.linalg.norm(r) / bar)
        k = int(np.argmax(rb / np.maximum(bb, 1e-300)))
        out.update(ratio=ratio, worst_block=(blocks[k][0], blocks[k][1]), block_ratio=float(rb[k] / max(bb[k], 1e-300)))
        if ratio > 1.0:
            raise DirectCertificateError("%s: |b - A d_s| = %.3e is %.3g x its bar %.3e; worst block row: %s %d (rows %d..%d), |r_a| = %.3e = %.3g x its bar"
                                         % (what, np.linalg.norm(r), ratio, bar, blocks[k][0], blocks[k][1], blocks[k][2], blocks[k][2] + blocks[k][3] - 1,
                                            rb[k], rb[k] / max(bb[k], 1e-300)))
    if rs.F and frame_part:
        if not np.all(np.isfinite(df)):
            raise DirectCertificateError((what, "the frame part is not finite"))
        ref = rs.backsub(ds_)
        scale = rs.backsub_scale(ds_)
        zsl = np.linalg.norm(zs) * ULP
        prop = np.linalg.norm(np.einsum("fij,efj->fie", rs.Vinv, rs.W64), axis=(1, 2)) * zsl
        err = np.linalg.norm(df - ref, axis=1)
        lim = 1e-10 * scale + ULP * np.linalg.norm(zf, axis=1) * 2 + prop * 2
        fr = err / np.maximum(lim, 1e-300)
        out["frame_ratio"] = float(fr.max())
        bad = np.nonzero(err > lim)[0]
        if len(bad):
            raise DirectCertificateError("%s: back-substitution: frame %d is %.3g x its bar (%d frames over)" % (what, bad[np.argmax(fr[bad])], fr[bad].max(), len(bad)))
    return out


# ---- the host reference: an unpivoted block LDL^T in 96-row tiles on the Schur complement summed in reverse frame order ----
def reduce_reverse(rs):
    """A, b with the frames' shares subtracted one by one, last frame first (plain float64)"""
    n = len(rs.ent)
    A = rs.U.copy()
    b = rs.gs.copy()
    for f in range(rs.F - 1, -1, -1):
        Wf = rs.W64[:, f, :]
        Y = Wf @ rs.Vinv[f]
        A -= Y @ Wf.T
        b -= Y @ rs.gf[f]
    he = rs.held_e
    A[he, :] = 0.0
    A[:, he] = 0.0
    A[he, he] = 1.0
    b[he] = 0.0
    return A, b


def _ldl_tile(T):
    """unpivoted LDL^T of one tile: (unit lower L, D)"""
    m = len(T)
    L = np.eye(m)
    D = np.zeros(m)
    T = T.copy()
    for j in range(m):
        D[j] = T[j, j]
        L[j + 1:, j] = T[j + 1:, j] / D[j]
        T[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], T[j + 1:, j])
    return L, D


def _lower_solve(L, X):
    """L^-1 X for a unit lower triangular L (forward substitution, row by row)"""
    X = X.copy()
    for i in range(1, len(L)):
        X[i] -= L[i, :i] @ X[:i]
    return X


def block_ldl_solve(A, b, nb=96):
    """solve A x = b by a right-looking unpivoted block LDL^T (only the lower triangle of A is read)"""
    n = len(b)
    S = np.tril(A).copy()
    y = b.copy()
    tiles = [(o, min(o + nb, n)) for o in range(0, n, nb)]
    Ls, Ds = [], []
    for o, e in tiles:
        T = S[o:e, o:e] + np.tril(S[o:e, o:e], -1).T
        L, D = _ldl_tile(T)
        Ls.append(L)
        Ds.append(D)
        if e < n:
            P = _lower_solve(L, S[e:, o:e].T).T            # (L_panel D) = A_panel L^-T
            Lp = P / D
            S[e:, o:e] = Lp
            S[e:, e:] -= np.tril(Lp @ P.T)
    # forward, diagonal, backward
    for (o, e), L in zip(tiles, Ls):
        y[o:e] = _lower_solve(L, y[o:e][:, None])[:, 0]
        y[e:] -= S[e:, o:e] @ y[o:e]
    for (o, e), D in zip(tiles, Ds):
        y[o:e] /= D
    for (o, e), L in reversed(list(zip(tiles, Ls))):
        y[o:e] -= S[e:, o:e].T @ y[e:]
        y[o:e] = _lower_solve(L.T[::-1, ::-1], y[o:e][::-1][:, None])[::-1, 0]
    return y
