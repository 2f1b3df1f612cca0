"""Float64 restatement of aar_problem_predict_corners / aar_problem_detection_leverage -- TEST INFRASTRUCTURE ONLY, numpy only.

For a query q = (camera c, marker m, frame f) the device forms C_q = G_q Sigma_q G_q^T, G_q = du_q / d(camera, marker, frame) (8 x 18) and
Sigma_q the 18 x 18 block of (J^T J)^-1 for the triple.  This module states the BLOCK route the kernel takes, on the restated reduced system of
tests/covariance_certificate.py (CovSystem: S at mu = 0, V_f^-1, W):

    Sigma_cc, Sigma_mm, Sigma_cm = blocks of S^-1
    Sigma_ff = V_f^-1 + G S^-1 G^T                      G = V_f^-1 W_f^T  (6 x n, the slots of frame f side by side)
    Sigma_fe = -G (S^-1)_{:, e}                          e in {c, m}

with the MASK RULE: a parameter that is a constant (root, non-optimised group, fixed by the caller, the frames of a problem that does not
optimise them) has zero rows and columns in Sigma_q -- the identity rows that S carries for them are read as zero --, and the covariance is
UNDEFINED (status bit 1) when frames are optimised and f has no detection, or c / m has a z column, is not held and nothing touches it.  J
comes from tests/projection_reference.py by the complex step, not from the closed form the kernels share.

The other route (dense): J_full H^-1 J_full^T with numpy.linalg.inv of H over its live rows.  The two are compared in the measure

    |C_a - C_b|_F / s_q,      s_q = | |J| |Sigma_q| |J^T| |_F

whose scale takes no credit for the cancellation between the camera and the frame (s_q / |C_q| is in the hundreds).

`fault` plants the mistakes a kernel of this shape can make: "no_cross" (Sigma_fe left out), "cross_sign" (+G S^-1), "held_identity" (the
identity rows of S^-1 read as they stand), "fm_for_fc" (Sigma_fm written where Sigma_fc belongs), "skip_slot" (one slot of the frame missing
from the cross sum).
"""
import numpy as np

import covariance_certificate as cc
import projection_reference as pr

BEHIND, UNDEFINED = 1, 2
FLAT_BAR = 1e-7          # the project's flat bar for a block of the covariance (tests/test_gpu_covariance.py)
FAULTS = ("no_cross", "cross_sign", "held_identity", "fm_for_fc", "skip_slot")


def query_projection(ds, x_full, q):
    """(uv [Q, 8], J [Q, 8, 18], depth [Q, 4]) of queries q [Q, 3] at x_full: the forward model and its complex-step derivative with respect
    to (camera 6, marker 6, frame 6), whether or not a group is optimised"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
    ref = pr.Reference(ds)
    cam, mk, fr = ref.entity_vectors(np.asarray(x_full, dtype=np.float64)[:6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1) + 6 * ds.num_frames])
    K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 3, 3)[q[:, 0]]
    base = [cam[q[:, 0]], mk[q[:, 1]], fr[q[:, 2]]]
    uv = pr.project(base[0], base[1], base[2], K, ref.h)
    depth = pr.camera_points(base[0], base[1], base[2], ref.h)[..., 2]
    J = np.empty((len(q), 8, 18))
    cb = [b.astype(np.complex128) for b in base]
    Kc = K.astype(np.complex128)
    for g in range(3):
        for k in range(6):
            args = list(cb)
            a = cb[g].copy()
            a[:, k] += 1j * pr.CSTEP
            args[g] = a
            J[:, :, 6 * g + k] = pr.project(args[0], args[1], args[2], Kc, ref.h).imag / pr.CSTEP
    return uv, J, depth


class PredictSystem:
    """The restatement bound to one problem: ds, its dense H (priors included through Hp) and the switches of the Problem."""

    def __init__(self, ds, H, optimize=(True, True, True), fixed_cams=(), fixed_markers=(), Hp=None):
        self.ds, self.optimize = ds, tuple(bool(b) for b in optimize)
        self.cs = cs = cc.CovSystem(ds, H, optimize, False, fixed_cams, fixed_markers, Hp)
        self.H = cs.H
        self.fixed_cams, self.fixed_markers = set(int(c) for c in fixed_cams), set(int(m) for m in fixed_markers)
        self.off = {(k, i): o for k, i, o, _ in cs.blocks}
        self.frame_pos = {int(f): k for k, f in enumerate(cs.frames_live)}
        n, lv = cs.n, cs.live
        self.Sinv = np.zeros((n, n))
        if lv.any():
            self.Sinv[np.ix_(lv, lv)] = np.linalg.inv(cs.rs.A64[np.ix_(lv, lv)])
        # the dense route: H^-1 over the rows with an unknown, and where each z column sits in it
        self.idx = np.r_[cs.ent[lv], cs.frame_idx]
        self.Hinv = np.linalg.inv(self.H[np.ix_(self.idx, self.idx)]) if len(self.idx) else np.zeros((0, 0))
        self.pos = {int(z): k for k, z in enumerate(self.idx)}
        self.num_live_vars = len(self.idx)
        self._frame_cache = {}

    # ---- what a parameter block of the triple is: ("const",) | ("unseen",) | ("live", first reduced unknown / live frame position)
    def entity_state(self, kind, i):
        ds = self.ds
        if kind == "camera":
            const = i == ds.root_cam or not self.optimize[0] or i in self.fixed_cams
        else:
            const = i == ds.root_marker or not self.optimize[1] or i in self.fixed_markers
        if const:
            return ("const",)
        o = self.off[(kind, i)]
        return ("live", o) if self.cs.live[o] else ("unseen",)

    def frame_state(self, f):
        if not self.optimize[2]:
            return ("const",)
        return ("live", self.frame_pos[f]) if f in self.frame_pos else ("unseen",)

    def gain(self, k):
        """(G = V_f^-1 W_f^T (6 x n), Sigma_ff) of live frame position k"""
        if k not in self._frame_cache:
            rs = self.cs.rs
            G = rs.Vinv[k] @ rs.W64[:, k, :].T
            self._frame_cache[k] = (G, rs.Vinv[k] + G @ self.Sinv @ G.T)
        return self._frame_cache[k]

    def sigma_block(self, c, m, f, fault=None):
        """Sigma_q (18 x 18) by the block route, or None where the covariance is undefined"""
        sc, sm, sf = self.entity_state("camera", c), self.entity_state("marker", m), self.frame_state(f)
        if "unseen" in (sc[0], sm[0], sf[0]):
            return None
        Sinv = self.Sinv
        if fault == "held_identity":
            Sinv = Sinv.copy()
            dead = ~self.cs.live
            Sinv[dead, dead] = 1.0
        S = np.zeros((18, 18))
        rows = {}
        for g, (kind, i, st) in enumerate((("camera", c, sc), ("marker", m, sm))):
            if st[0] == "live":
                rows[g] = np.arange(st[1], st[1] + 6)
            elif fault == "held_identity" and (kind, i) in self.off:          # a held entity's rows read as they stand
                rows[g] = np.arange(self.off[(kind, i)], self.off[(kind, i)] + 6)
        for g in rows:
            for h in rows:
                S[6 * g:6 * g + 6, 6 * h:6 * h + 6] = Sinv[np.ix_(rows[g], rows[h])]
        if sf[0] == "live":
            k = sf[1]
            rs = self.cs.rs
            G, S[12:, 12:] = self.gain(k)
            Gx = G
            if fault == "skip_slot":
                seen = np.nonzero(np.abs(rs.W64[:, k, :]).sum(axis=1))[0]
                Gx = G.copy()
                if len(seen):
                    e0 = 6 * (seen[len(seen) // 2] // 6)
                    Gx[:, e0:e0 + 6] = 0.0
            cross = {g: -Gx @ Sinv[:, rows[g]] for g in rows}
            if fault == "cross_sign":
                cross = {g: -v for g, v in cross.items()}
            if fault == "no_cross":
                cross = {}
            if fault == "fm_for_fc" and 0 in cross and 1 in cross:
                cross[0] = cross[1]
            for g, v in cross.items():
                S[12:, 6 * g:6 * g + 6] = v
                S[6 * g:6 * g + 6, 12:] = v.T
        return S

    def z_columns(self, c, m, f):
        """z column of each of the 18 parameters of the triple, -1 where it has none or is held / dead"""
        ds = self.ds
        col = np.full(18, -1, dtype=np.int64)
        oc, om, of = self.optimize
        nc = 6 * (ds.num_cams - 1) if oc else 0
        nm = 6 * (ds.num_markers - 1) if om else 0
        if self.entity_state("camera", c)[0] == "live":
            col[0:6] = 6 * (c - (c > ds.root_cam)) + np.arange(6)
        if self.entity_state("marker", m)[0] == "live":
            col[6:12] = nc + 6 * (m - (m > ds.root_marker)) + np.arange(6)
        if self.frame_state(f)[0] == "live":
            col[12:18] = nc + nm + 6 * f + np.arange(6)
        return col

    def sigma_dense(self, c, m, f):
        """Sigma_q from numpy.linalg.inv of H over its live rows; None where undefined"""
        if "unseen" in (self.entity_state("camera", c)[0], self.entity_state("marker", m)[0], self.frame_state(f)[0]):
            return None
        col = self.z_columns(c, m, f)
        S = np.zeros((18, 18))
        ok = np.nonzero(col >= 0)[0]
        p = np.array([self.pos[int(z)] for z in col[ok]], dtype=np.int64)
        if len(ok):
            S[np.ix_(ok, ok)] = self.Hinv[np.ix_(p, p)]
        return S

    def status(self, q, depth):
        q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
        st = np.zeros(len(q), dtype=np.uint8)
        st[~(depth > 0).all(axis=1)] |= BEHIND
        for i, (c, m, f) in enumerate(q):
            if "unseen" in (self.entity_state("camera", c)[0], self.entity_state("marker", m)[0], self.frame_state(f)[0]):
                st[i] |= UNDEFINED
        return st


U53 = 2.0 ** -53


def with_device_blocks(ps, entity_cov, frames):
    """A copy of ps whose block route reads what the DEVICE returned: Problem.covariance(dense=True).entity_cov for S^-1 (its NaN rows read as
    zero) and .frames for Sigma_ff; the gains G_a^(f) = V_f^-1 W_a^T come from the H the system was built from (the device's
    eval_normal_equations).  The NaN pattern of entity_cov must be the system's rows without an unknown."""
    import copy
    entity_cov = np.asarray(entity_cov, dtype=np.float64)
    assert entity_cov.shape == ps.Sinv.shape
    assert np.array_equal(np.isnan(entity_cov), ps.cs.nan_pattern()), "NaN pattern of the device's entity covariance"
    ref = copy.copy(ps)
    ref.Sinv = np.nan_to_num(entity_cov)
    ref._frame_cache = {}
    rs = ps.cs.rs
    for k, f in enumerate(ps.cs.frames_live):
        blk = np.asarray(frames[f], dtype=np.float64).reshape(6, 6)
        assert np.isfinite(blk).all(), "frame %d has detections and no finite block" % f
        ref._frame_cache[k] = (rs.Vinv[k] @ rs.W64[:, k, :].T, blk)
    return ref


def certificate_bars(ps, q, s):
    """gamma_q kappa_f s_q + 2 SCALED_BAR s_q per query.  gamma_q counts the rounded operations of k_predict_corners behind one entry of C_q
    beyond what the reference shares with it: an entry of Sigma_fe is a sum of 6 k_f products in slot order (6 k_f), every gain entry a
    six-term sum with V_f^-1 (6) whose own elimination costs at most 2 * 6 operations per entry (12), relative to kappa_f = cond_2(V_f); the
    two 18-term products T = G Sigma and C = T G^T add 36:   gamma_q = (6 k_f + 18 + 36) 2^-53   (k_f = 0, kappa_f = 1 where the frames are
    constants).  The second term is the closed-form Jacobian of the kernel against the complex step, which enters C twice."""
    conds = ps.cs.rs.frame_conds() if ps.cs.rs.F else np.zeros(0)
    out = np.empty(len(q))
    for i, (c, m, f) in enumerate(np.asarray(q, dtype=np.int64).reshape(-1, 3)):
        st = ps.frame_state(int(f))
        kf, kap = (int(ps.cs.kf[st[1]]), float(conds[st[1]])) if st[0] == "live" else (0, 1.0)
        out[i] = ((6 * kf + 18 + 36) * U53 * kap + 2 * pr.SCALED_BAR) * s[i]
    return out


def push(J, S):
    """C = J Sigma J^T and its scale s = | |J| |Sigma| |J^T| |_F"""
    return J @ S @ J.T, float(np.linalg.norm(np.abs(J) @ np.abs(S) @ np.abs(J).T))


def covariances(ps, x_full, q, route="block", fault=None):
    """(C [Q, 8, 8] NaN where undefined or behind, s [Q], uv [Q, 8] NaN where behind, status [Q]) of queries q"""
    q = np.asarray(q, dtype=np.int64).reshape(-1, 3)
    uv, J, depth = query_projection(ps.ds, x_full, q)
    st = ps.status(q, depth)
    C = np.full((len(q), 8, 8), np.nan)
    s = np.full(len(q), np.nan)
    for i, (c, m, f) in enumerate(q):
        if st[i]:
            continue
        S = ps.sigma_block(int(c), int(m), int(f), fault) if route == "block" else ps.sigma_dense(int(c), int(m), int(f))
        C[i], s[i] = push(J[i], S)
    uv = uv.copy()
    uv[(st & BEHIND) != 0] = np.nan
    return C, s, uv, st


def detection_queries(ds):
    return np.stack([np.asarray(ds.obs_cam), np.asarray(ds.obs_marker), np.asarray(ds.obs_frame)], axis=1).astype(np.int64)


def frame_grid_queries(ds, frames):
    """every (camera, marker) of the given frames"""
    c, m = np.meshgrid(np.arange(ds.num_cams), np.arange(ds.num_markers), indexing="ij")
    return np.concatenate([np.stack([c.reshape(-1), m.reshape(-1), np.full(c.size, f)], axis=1) for f in frames]).astype(np.int64)


def three_frames(ds):
    """first, middle and last frame"""
    F = int(ds.num_frames)
    return sorted(set([0, F // 2, F - 1]))


def trace_tree(C):
    """the trace in the kernel's order: ((d0 + d1) + (d2 + d3)) + ((d4 + d5) + (d6 + d7))"""
    d = np.diagonal(np.asarray(C), axis1=-2, axis2=-1)
    return ((d[..., 0] + d[..., 1]) + (d[..., 2] + d[..., 3])) + ((d[..., 4] + d[..., 5]) + (d[..., 6] + d[..., 7]))
