"""Certificate of aar_problem_covariance (k_frame_inv -> k_schur* -> k_cov_stage -> k_ldl_* -> k_cov_gather -> k_cov_linv_* -> k_cov_sinv ->
k_cov_frames) -- TEST INFRASTRUCTURE ONLY, numpy only (direct_cases.frame_entity_counts counts the slots).

The call inverts the reduced system of the device's own dense normal equations at mu = 0, so the certificate takes H from
Problem.eval_normal_equations (the device's H carries the Huber weights and the pose priors' blocks already; the oracle's takes the priors as Hp)
and restates only what the chain does (tests/reduced_system.py at mu = 0, tests/direct_certificate.py for the z-order bookkeeping):

    S = U - sum_f W_f V_f^-1 W_f^T        Sigma_ee = S^-1        Sigma_ff = V_f^-1 + sum_{a,b} G_a Sigma_ab G_b^T,  G_a = V_f^-1 W_a^T

Rows without an unknown -- caller-fixed entities, rows of H that are identically zero (an entity no detection touches, the five distortion
columns of an intrinsics entity) -- are identity rows of S, as on the device; a frame without detections has no block.  "Live" rows are the rest.

(a) entity part.  Sigma* = S^-1 over the live rows: numpy's inverse of the float64 S, refined once with the residual I - S Sigma taken in
    np.longdouble and kept in np.longdouble.  Premise, asserted before anything is compared: |Sigma*| |I - S Sigma*|, the first-order error of
    Sigma* itself, is below 1/64 of the bar in every block (1/4 where np.longdouble is no wider than float64).  Then, per block (a, b) of the
    entities (6 x 6; the live 4 x 4 of an intrinsics entity):

        |(Sigma_dev - Sigma*)_ab|_F <= gamma |(|Sigma*| M |Sigma*|)_ab|_F
        M     = |U| + sum_f kappa_f |W_f| |V_f^-1| |W_f^T|  +  |L| |D| |L^T|          kappa_f = cond_2(V_f)
        gamma = ((3 n + 12 F_max + 64) + (n + 32) + (n + 2)) 2^-53                     n: entity unknowns, F_max: the most frames any entity is seen in

    The first-order error of an inverse is Sigma dS Sigma, with dS what the chain's S and its factor are off by: the first term of M is what the
    entries of S add up to in absolute value (ReducedSystem.abs_sums: every frame's share weighted with the condition of the block inverted for
    it), the second is the backward error of an unpivoted LDL^T (L, D of a float64 LDL^T in 96-row tiles of the restated S).  gamma is an
    operation count: 3 n + 12 F_max + 64 is the formation and factorisation as in the direct chain's certificate (a block of S seen in F_max
    frames is a sum of 6 F_max six-term products formed twice, the factorisation adds at most 3 n rounded operations per entry); an entry of
    X = L^-1 is a sum of at most n products (X_IJ = -X_II sum_K L_IK X_KJ) times a 32-term product with X_II: n + 32; an entry of X^T D^-1 X is a
    sum of at most n products, each with one division and one scaling: n + 2.  Nothing is fitted to what a kernel gives.
    A failure names the worst block by entity kind and index, and gives its ratio; it also names the block in which S Sigma_dev S - S, the error
    carried back to S, is largest: a wrong block of S or of L spreads over all of Sigma and stays in place there.
(b) frame part.  Reference: V_f^-1 + G_f Sigma_dev G_f^T in float64 with the entity covariance the DEVICE returned (its NaN rows read as zero,
    as k_cov_frames reads them), so that the error of (a) is not charged twice.  Per frame

        |Sigma_ff,dev - ref|_F <= gamma_f kappa_f | |V_f^-1| + |G_f| |Sigma_dev| |G_f^T| |_F
        gamma_f = (12 ceil(P_f / 64) + 6 + 3 + 3 * 18) 2^-53         P_f = k_f (k_f + 1) / 2 slot pairs, k_f the frame's slots

    a lane adds ceil(P_f / 64) pairs, each through two six-term FMA sums (12); the butterfly over the wavefront adds 6, the transpose, the
    diagonal's half and V_f^-1 add 3; V_f^-1 enters three times (alone and inside both G), each time through a six-term sum (6) with the
    inverse's own elimination (at most 2 * 6 operations per entry), relative to kappa_f.  A frame without detections is NaN on both sides.
(c) patterns: NaN exactly where a row has no unknown; sigma2 and sum_sq to rtol 1e-12 of the device's own sum of squares; min_pivot and
    max_pivot each within gamma cond_2(S) (relative) of min D and of max D of the restated LDL^T over the live rows -- tighter than the pivot
    range as a whole, which a max_pivot reported as min_pivot would still meet.

What the bar does not see (block_resolution): a relative error in ONE block (a, b) of Sigma below eps* = bar_ab / |Sigma*_ab|_F.
"""
import numpy as np

from direct_cases import frame_entity_counts
from direct_certificate import U53, WIDE, _ldl_tile, _lower_solve, entity_blocks, reduce_reverse
from reduced_system import ReducedSystem, held_mask, split_indices

LD = np.longdouble
PREMISE = 1.0 / 64 if WIDE else 0.25


class CovarianceCertificateError(AssertionError):
    pass


def block_ldl(A, nb=96):
    """unpivoted LDL^T of A in nb-row tiles, right-looking (only the lower triangle is read): (dense unit lower L, D)"""
    n = len(A)
    S = np.tril(A).copy()
    L = np.eye(n)
    D = np.zeros(n)
    for o in range(0, n, nb):
        e = min(o + nb, n)
        Lt, Dt = _ldl_tile(S[o:e, o:e] + np.tril(S[o:e, o:e], -1).T)
        L[o:e, o:e] = Lt
        D[o:e] = Dt
        if e < n:
            Pn = _lower_solve(Lt, S[e:, o:e].T).T
            Lp = Pn / Dt
            L[e:, o:e] = Lp
            S[e:, e:] -= np.tril(Lp @ Pn.T)
    return L, D


def _slices(A, beta, k, axis):
    """A as k slices of at most beta bits each, counted from the largest entry of every row (axis = 1) or column (axis = 0): slice s is a multiple
    of 2^(e + 1 - (s + 1) beta) no larger than 2^(e - s beta), 2^e >= the row's largest entry; what is left is below 2^(e - k beta)"""
    mx = np.abs(A).max(axis=axis, keepdims=True)
    e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
    R = np.array(A, dtype=np.float64)
    out = []
    for s in range(k):
        sg = 1.5 * 2.0 ** (e + 53 - (s + 1) * beta)
        T = (R + sg) - sg
        out.append(T)
        R = R - T
    return out


def matmul_wide(A, B, k=4):
    """(A @ B in np.longdouble, bound of what it is off by) for float64 A, B: both are cut into k slices whose products float64 sums exactly,
    whatever the order (2 beta + log2 n <= 53), the products of the leading slices are added in np.longdouble.  A plain np.longdouble matmul is
    the same to rounding and takes a minute at 1 300 unknowns."""
    n = A.shape[1]
    beta = int((53 - np.ceil(np.log2(max(n, 2)))) // 2)
    As, Bs = _slices(A, beta, k, 1), _slices(B, beta, k, 0)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for p in range(k):
        for q in range(k - p):
            acc += (As[p] @ Bs[q]).astype(LD)
    aa, ab = np.abs(A), np.abs(B)
    off = 16 * float(np.finfo(LD).eps) * (aa @ ab) + 4 * (k + 1) * n * 2.0 ** (-k * beta) * aa.max(axis=1, keepdims=True) * ab.max(axis=0, keepdims=True)
    return acc, off


class CovSystem:
    """The float64 restatement of one problem's covariance: rs (ReducedSystem at mu = 0 over the frames that have detections), blocks
    (direct_certificate.entity_blocks), live (mask of the entity unknowns that carry an unknown), frames_live (indices of the frames with a
    block), kf (slots per frame)."""

    def __init__(self, ds, H, optimize=(True, True, True), intrinsics=False, fixed_cams=(), fixed_markers=(), Hp=None):
        H = np.array(H, dtype=np.float64)
        if Hp is not None:
            H += Hp
        P = len(H)
        ent, frames = split_indices(ds, optimize, intrinsics)
        dead = ~np.abs(H).sum(axis=1).astype(bool)
        held = held_mask(ds, P, fixed_cams, fixed_markers)
        held[ent] = held[ent] | dead[ent]
        self.nF = len(frames) // 6
        fd = dead[frames].reshape(self.nF, 6)
        assert np.all(fd.all(axis=1) == fd.any(axis=1)), "a frame with some dead rows"
        self.frames_live = np.nonzero(~fd.all(axis=1))[0]
        fidx = frames.reshape(self.nF, 6)[self.frames_live].reshape(-1)
        self.rs = ReducedSystem(H, np.zeros(P), 0.0, ent, fidx, held=held)
        self.H, self.ent, self.frame_idx = H, ent, fidx
        self.blocks = entity_blocks(ds, optimize, intrinsics)
        self.live = ~self.rs.held_e
        self.n = len(ent)
        self.kf = np.array(frame_entity_counts(ds, intrinsics), dtype=int)[self.frames_live] if self.nF else np.zeros(0, int)
        self._starts = np.array([b[2] for b in self.blocks], dtype=int)
        assert not self.blocks or self.blocks[-1][2] + self.blocks[-1][3] == self.n

    # ---- the entity part ----
    def gamma(self):
        rs = self.rs
        fmax = int(rs.frames_seen().max()) if self.n else 0
        return ((3 * self.n + 12 * fmax + 64) + (self.n + 32) + (self.n + 2)) * U53

    def block_norms(self, Ml):
        """Frobenius norms [blocks][blocks] of a matrix over the live rows"""
        full = np.zeros((self.n, self.n))
        full[np.ix_(self.live, self.live)] = np.asarray(Ml, dtype=np.float64) ** 2
        return np.sqrt(np.add.reduceat(np.add.reduceat(full, self._starts, axis=0), self._starts, axis=1))

    def entity(self):
        """dict(sigma: Sigma* [live][live] in np.longdouble, bars, premise: block norms of Sigma*'s own first-order error, D, cond)"""
        if not hasattr(self, "_ent"):
            lv = self.live
            Sl = self.rs.A64[np.ix_(lv, lv)]
            S0 = np.linalg.inv(Sl)
            S0 = 0.5 * (S0 + S0.T)
            eye = np.eye(len(Sl), dtype=LD)
            P0, off0 = matmul_wide(Sl, S0)
            corr = S0 @ np.asarray(eye - P0, dtype=np.float64)
            corr = 0.5 * (corr + corr.T)
            sig = S0.astype(LD) + corr.astype(LD)                      # (its rounding to np.longdouble is inside off0)
            P1, off1 = matmul_wide(Sl, corr, k=2)
            R = np.abs(np.asarray((eye - P0) - P1, dtype=np.float64)) + off0 + off1
            if not WIDE:
                R += len(Sl) * U53 * (np.abs(Sl) @ np.abs(S0))
            sa = np.abs(np.asarray(sig, dtype=np.float64))
            L, D = block_ldl(self.rs.A64)
            M = self.rs.abs_sums()[0] + (np.abs(L) * np.abs(D)) @ np.abs(L).T
            self.M = M
            bars = self.gamma() * self.block_norms(sa @ M[np.ix_(lv, lv)] @ sa)
            ev = np.linalg.eigvalsh(Sl)
            self._ent = dict(sigma=sig, bars=bars, premise=self.block_norms(sa @ R), D=D[lv], cond=float(ev[-1] / ev[0]), lmin=float(ev[0]),
                             norms=self.block_norms(sa))
        return self._ent

    def nan_pattern(self):
        m = np.zeros((self.n, self.n), bool)
        m[~self.live, :] = True
        m[:, ~self.live] = True
        return m

    def block_resolution(self, i, j):
        """eps*: the relative error of block (i, j) of Sigma at which that block's ratio reaches 1"""
        e = self.entity()
        return float(e["bars"][i, j] / max(e["norms"][i, j], 1e-300))


def certify_entity(cs, sigma_dev, what=""):
    """assert the premise, the NaN pattern and (a) for a dense entity covariance in z entity order.  Returns dict(ratio, worst_block, premise)."""
    e = cs.entity()
    ok = e["bars"] > 0
    prem = float((e["premise"][ok] / e["bars"][ok]).max()) if ok.any() else 0.0
    assert prem <= PREMISE, "%s: PREMISE: the reference's own error is %.3g of the bar (limit %.3g)" % (what, prem, PREMISE)
    sigma_dev = np.asarray(sigma_dev, dtype=np.float64)
    if sigma_dev.shape != (cs.n, cs.n):
        raise CovarianceCertificateError("%s: entity covariance of shape %s, expected %d x %d" % (what, sigma_dev.shape, cs.n, cs.n))
    if not np.array_equal(np.isnan(sigma_dev), cs.nan_pattern()):
        bad = np.nonzero(np.isnan(sigma_dev) != cs.nan_pattern())
        raise CovarianceCertificateError("%s: NaN pattern differs at %d entries, first (%d, %d)" % (what, len(bad[0]), bad[0][0], bad[1][0]))
    lv = cs.live
    dl = sigma_dev[np.ix_(lv, lv)]
    if not np.all(np.isfinite(dl)):
        raise CovarianceCertificateError("%s: the entity covariance is not finite" % what)
    err = cs.block_norms(np.asarray(dl.astype(LD) - e["sigma"], dtype=np.float64))
    ratio = np.where(ok, err / np.where(ok, e["bars"], 1.0), np.where(err > 0, np.inf, 0.0))
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    out = dict(ratio=float(ratio[i, j]), worst_block=(cs.blocks[i][:2], cs.blocks[j][:2]), premise=prem)
    if out["ratio"] > 1.0:
        # where in S the error sits: S Sigma_dev S - S is -dS to first order (plain float64: a diagnostic, not a bar), per block relative to
        # (|S_aa| |S_bb|)^1/2 -- an error of one block of S or of its factor spreads over all of Sigma, and stays where it is in here
        Sl = cs.rs.A64[np.ix_(lv, lv)]
        back = cs.block_norms(Sl @ dl @ Sl - Sl)
        dn = np.sqrt(np.maximum(np.diag(cs.block_norms(Sl)), 1e-300))
        p, q = np.unravel_index(int(np.argmax(back / np.outer(dn, dn))), back.shape)
        err_ = CovarianceCertificateError("%s: worst block: (%s %d, %s %d), |Sigma_dev - Sigma*| = %.3e is %.3g x its bar %.3e (%d of %d blocks over); "
                                         "backward error S Sigma S - S largest in block: (%s %d, %s %d)"
                                         % (what, cs.blocks[i][0], cs.blocks[i][1], cs.blocks[j][0], cs.blocks[j][1], err[i, j], ratio[i, j],
                                            e["bars"][i, j], int((ratio > 1).sum()), ratio.size,
                                            cs.blocks[p][0], cs.blocks[p][1], cs.blocks[q][0], cs.blocks[q][1]))
        err_.ratios = ratio                    # [blocks][blocks], for a caller that wants the extent of the damage
        raise err_
    return out


def frame_gamma(kf):
    pf = kf * (kf + 1) // 2
    return (12 * -(-pf // 64) + 6 + 3 + 3 * 18) * U53


def frame_reference(cs, sigma_dev):
    """(ref [Fl][6][6], bars [Fl]) of the frames with a block, from the entity covariance sigma_dev (NaN read as zero)"""
    rs = cs.rs
    sg = np.nan_to_num(np.asarray(sigma_dev, dtype=np.float64))
    G = np.einsum("fij,efj->fie", rs.Vinv, rs.W64)
    ref = rs.Vinv + np.einsum("fie,fje->fij", G @ sg, G)
    Ga = np.abs(G)
    mag = np.abs(rs.Vinv) + np.einsum("fie,fje->fij", Ga @ np.abs(sg), Ga)
    bars = frame_gamma(cs.kf) * rs.frame_conds() * np.linalg.norm(mag, axis=(1, 2))
    return ref, bars


def certify_frames(cs, sigma_dev, frames_dev, what="", partial=False):
    """assert (b) for frames_dev [F][6][6] against the frame formula on sigma_dev.  partial: a sharded rank, whose other ranks' frames are NaN and
    skipped.  Returns dict(ratio, worst_frame, certified: indices of the frames that were compared)."""
    frames_dev = np.asarray(frames_dev, dtype=np.float64).reshape(-1, 6, 6)
    if len(frames_dev) != cs.nF:
        raise CovarianceCertificateError("%s: %d frame blocks, expected %d" % (what, len(frames_dev), cs.nF))
    out = dict(ratio=0.0, worst_frame=None, certified=[])
    allnan = np.isnan(frames_dev).all(axis=(1, 2))
    fin = np.isfinite(frames_dev).all(axis=(1, 2))
    empty = np.ones(cs.nF, bool)
    empty[cs.frames_live] = False
    if not np.all(allnan[empty]):
        raise CovarianceCertificateError("%s: frame %d has no detections and a block that is not NaN" % (what, np.nonzero(empty & ~allnan)[0][0]))
    if not cs.rs.F:
        return out
    ref, bars = frame_reference(cs, sigma_dev)
    for k, f in enumerate(cs.frames_live):
        if partial and allnan[f]:
            continue
        if not fin[f]:
            raise CovarianceCertificateError("%s: frame %d: the block is not finite" % (what, f))
        r = float(np.linalg.norm(frames_dev[f] - ref[k]) / bars[k])
        out["certified"].append(int(f))
        if r > out["ratio"]:
            out.update(ratio=r, worst_frame=int(f))
    if out["ratio"] > 1.0:
        raise CovarianceCertificateError("%s: worst frame: %d (%d slots), |Sigma_ff - ref| is %.3g x its bar" % (what, out["worst_frame"],
                                         cs.kf[list(cs.frames_live).index(out["worst_frame"])], out["ratio"]))
    return out


def certify_report(cs, cv, sum_sq, num_vars, num_residuals, what=""):
    """(c): sigma2, sum_sq and the pivot range of a Covariance against the device's own sum of squares and the restated LDL^T"""
    e = cs.entity()
    np.testing.assert_allclose(cv.sum_sq, sum_sq, rtol=1e-12, err_msg=what)
    np.testing.assert_allclose(cv.sigma2, sum_sq / (num_residuals - num_vars), rtol=1e-12, err_msg=what)
    g = cs.gamma() * e["cond"]
    lo, hi = e["D"].min(), e["D"].max()
    if not (abs(cv.min_pivot - lo) <= g * lo and abs(cv.max_pivot - hi) <= g * hi):
        raise CovarianceCertificateError("%s: pivots %.17g .. %.17g outside the restated %.17g .. %.17g (1 +- %.3g)" % (what, cv.min_pivot, cv.max_pivot, lo, hi, g))


# ---- the host restatement of the device's method: tile LDL^T of the reverse-order Schur complement, X = L^-1 by block rows, X^T D^-1 X ----
def linv_by_block_rows(L, ct=32):
    """X = L^-1 of a unit lower L: the ct x ct diagonal inverses, then block row I as X_IJ = -X_II sum_{K=J}^{I-1} L_IK X_KJ"""
    n = len(L)
    X = np.zeros((n, n))
    bl = [(o, min(o + ct, n)) for o in range(0, n, ct)]
    for o, e in bl:
        X[o:e, o:e] = _lower_solve(L[o:e, o:e], np.eye(e - o))
    for I, (o, e) in enumerate(bl):
        for J in range(I):
            oj, ej = bl[J]
            X[o:e, oj:ej] = -X[o:e, o:e] @ (L[o:e, oj:o] @ X[oj:o, oj:ej])
    return X


def device_method(cs, L=None, D=None):
    """Sigma over the entity unknowns (NaN where no unknown) by the device's method in float64"""
    if L is None:
        A, _ = reduce_reverse(cs.rs)
        L, D = block_ldl(A)
    X = linv_by_block_rows(L)
    sg = (X.T / D) @ X
    sg = np.tril(sg) + np.tril(sg, -1).T
    sg[cs.nan_pattern()] = np.nan
    return sg


def frames_by_solves(cs, sigma, W=None):
    """the frame formula with np.linalg.solve instead of V^-1, last frame first: [F][6][6], NaN for the frames without detections"""
    rs = cs.rs
    W = rs.W64 if W is None else W
    sg = np.nan_to_num(sigma)
    out = np.full((cs.nF, 6, 6), np.nan)
    for k in range(rs.F - 1, -1, -1):
        G = np.linalg.solve(rs.V[k], W[:, k, :].T)
        out[cs.frames_live[k]] = np.linalg.solve(rs.V[k], np.eye(6)) + G @ sg @ G.T
    return out


def dense_inverse_route(cs):
    """(Sigma over the entity unknowns, frame blocks) from np.linalg.inv of the whole H over its rows with an unknown"""
    idx = np.r_[cs.ent[cs.live], cs.frame_idx]
    Hi = np.linalg.inv(cs.H[np.ix_(idx, idx)])
    nl = int(cs.live.sum())
    sg = np.full((cs.n, cs.n), np.nan)
    sg[np.ix_(cs.live, cs.live)] = Hi[:nl, :nl]
    fr = np.full((cs.nF, 6, 6), np.nan)
    for k, f in enumerate(cs.frames_live):
        fr[f] = Hi[nl + 6 * k:nl + 6 * k + 6, nl + 6 * k:nl + 6 * k + 6]
    return sg, fr
