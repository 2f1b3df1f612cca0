"""numpy restatement of the damped reduced (Schur) system the inexact solvers work on -- TEST INFRASTRUCTURE ONLY.

From the oracle's dense normal equations H, B (tests/oracle_lib.py, Oracle.normal_equations) and a damping mu, in float64:

    H + mu I  (+ the pose priors' blocks, added after the damping, as the device adds them behind pass B)
    A = U - sum_f W_f (V_f)^-1 W_f^T          U, V_f, W_f: the entity, frame and coupling blocks of the damped matrix
    b = g_s - sum_f W_f (V_f)^-1 g_f
    delta_f = (V_f)^-1 (g_f - W_f^T delta_s)    (the frame back-substitution)

Entity unknowns are the z-order cameras, markers and intrinsics (Problem.entity_block_sizes()); frame unknowns are six per frame.  Held
(fixed) entries are identity rows with a zero right-hand side, as in the kernels.  w32=True rounds every W block to fp32 (round to nearest) and
keeps every product and sum in fp64: the operator and right-hand side k_pcgf<true, .> works with (pcg_kernels.hip, pcgf_operator).

Also the pose-prior restatement (include/aar.h): prior_terms() gives the dense blocks the priors add.
"""
import numpy as np


# ---- the pose priors ----
def hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = hat(w / th)
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def so3_log(Q):
    v = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    s2 = np.linalg.norm(v)
    th = np.arctan2(0.5 * s2, 0.5 * (np.trace(Q) - 1))
    return v * (0.5 if s2 == 0 else th / s2)


def jl(w):
    th = np.linalg.norm(w)
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + 0.5 * K
    return np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K


def jr_inv(phi):
    th = np.linalg.norm(phi)
    K = hat(phi)
    k = 1 / 12 if th < 1e-8 else 1 / th ** 2 - (1 + np.cos(th)) / (2 * th * np.sin(th))
    return np.eye(3) + 0.5 * K + k * K @ K


def prior_e(x6, xp):
    return np.r_[so3_log(rodrigues(xp[:3]).T @ rodrigues(x6[:3])), x6[3:] - xp[3:]]


def prior_J(x6, xp):
    phi = prior_e(x6, xp)[:3]
    J = np.eye(6)
    J[:3, :3] = jr_inv(phi) @ jl(x6[:3]).T
    return J


def slot_col(ds, kind, idx):
    """z / x_full column of a camera or marker's 6-vector (default Config: cameras | markers | frames, roots skipped)"""
    if kind == "camera":
        return 6 * (idx - (idx > ds.root_cam))
    return 6 * (ds.num_cams - 1) + 6 * (idx - (idx > ds.root_marker))


def prior_terms(ds, x, priors, P):
    """dense J_p^T L J_p (P x P), -J_p^T L e, sum e^T L e of the priors at x"""
    H = np.zeros((P, P))
    B = np.zeros(P)
    cost = 0.0
    for kind, idx, xp, info in priors:
        c = slot_col(ds, kind, idx)
        x6 = x[c:c + 6]
        e = prior_e(x6, xp)
        J = prior_J(x6, xp)
        H[c:c + 6, c:c + 6] += J.T @ info @ J
        B[c:c + 6] -= J.T @ info @ e
        cost += e @ info @ e
    return H, B, cost


# ---- the z layout ----
def split_indices(ds, optimize=(True, True, True), intrinsics=False):
    """(entity indices, frame indices) into z: cameras | markers | frames | intrinsics (oracle/ba_oracle.cpp, Layout); the entity unknowns are
    the cameras', markers' and intrinsics' in that order (Problem.entity_block_sizes()), the frame unknowns six per frame"""
    oc, om, of = optimize
    nc = 6 * (ds.num_cams - 1) if oc else 0
    nm = 6 * (ds.num_markers - 1) if om else 0
    nf = 6 * ds.num_frames if of else 0
    ni = 9 * ds.num_cams if intrinsics else 0
    ent = np.r_[np.arange(nc + nm), nc + nm + nf + np.arange(ni)].astype(np.int64)
    frames = (nc + nm + np.arange(nf)).astype(np.int64)
    return ent, frames


def held_mask(ds, P, fixed_cams=(), fixed_markers=()):
    """z mask of the unknowns of caller-fixed cameras / markers (roots have none)"""
    h = np.zeros(P, bool)
    for c in fixed_cams:
        if c != ds.root_cam:
            h[slot_col(ds, "camera", c):slot_col(ds, "camera", c) + 6] = True
    for m in fixed_markers:
        if m != ds.root_marker:
            h[slot_col(ds, "marker", m):slot_col(ds, "marker", m) + 6] = True
    return h


class ReducedSystem:
    """The damped reduced system of (H, B) at mu.  ent / frames: index arrays into z (split_indices); held: z mask of fixed unknowns;
    Hp, Bp: pose-prior blocks added after the damping; w32: W blocks rounded to fp32."""

    def __init__(self, H, B, mu, ent, frames, held=None, Hp=None, Bp=None, w32=False):
        P = len(B)
        Hd = np.array(H, dtype=np.float64)
        Hd[np.diag_indices(P)] += mu
        g = np.array(B, dtype=np.float64)
        if Hp is not None:
            Hd += Hp
        if Bp is not None:
            g += Bp
        held = np.zeros(P, bool) if held is None else np.asarray(held, bool)
        self.P, self.mu, self.ent, self.frames, self.w32 = P, mu, np.asarray(ent), np.asarray(frames), w32
        assert len(self.frames) % 6 == 0
        self.F = len(self.frames) // 6
        he = held[self.ent]
        assert not held[self.frames].any()
        self.held_e = he
        U = Hd[np.ix_(self.ent, self.ent)]
        W = Hd[np.ix_(self.ent, self.frames)]
        W[he, :] = 0.0                                # (a fixed entity's delta is zero: its coupling never enters)
        U[he, :] = 0.0
        U[:, he] = 0.0
        U[he, he] = 1.0
        gs = g[self.ent].copy()
        gs[he] = 0.0
        gf = g[self.frames].reshape(self.F, 6)
        V = np.stack([Hd[np.ix_(self.frames[6 * f:6 * f + 6], self.frames[6 * f:6 * f + 6])] for f in range(self.F)]) if self.F else np.zeros((0, 6, 6))
        if self.F:
            off = Hd[np.ix_(self.frames, self.frames)].copy()
            for f in range(self.F):
                off[6 * f:6 * f + 6, 6 * f:6 * f + 6] = 0.0
            assert not off.any(), "frame unknowns couple with each other: not the bundle-adjustment structure"
        self.U, self.gs, self.gf, self.V = U, gs, gf, V
        self.Vinv = np.linalg.inv(V) if self.F else V
        self.W64 = W.reshape(len(self.ent), self.F, 6)
        self.W32 = self.W64.astype(np.float32).astype(np.float64)
        self.A64, self.b64 = self._reduce(self.W64)
        self.A32, self.b32 = self._reduce(self.W32)
        self.A, self.b = (self.A32, self.b32) if w32 else (self.A64, self.b64)

    def _reduce(self, W):
        T = np.einsum("efi,fij->efj", W, self.Vinv)                 # W_f V_f^-1
        n = len(self.ent)
        A = self.U - T.reshape(n, 6 * self.F) @ W.reshape(n, 6 * self.F).T
        b = self.gs - np.einsum("efj,fj->e", T, self.gf)
        he = self.held_e
        A[he, :] = 0.0
        A[:, he] = 0.0
        A[he, he] = 1.0
        b[he] = 0.0
        return 0.5 * (A + A.T), b

    # ---- solutions ----
    def solve_s(self, w32=None):
        A, b = self._pick(w32)
        return np.linalg.solve(A, b) if len(b) else b.copy()

    def backsub(self, ds_, w32=None):
        """delta_f = V_f^-1 (g_f - W_f^T delta_s), [F][6]"""
        W = self.W32 if (self.w32 if w32 is None else w32) else self.W64
        return np.einsum("fij,fj->fi", self.Vinv, self.gf - np.einsum("efj,e->fj", W, ds_))

    def backsub_scale(self, ds_, w32=None):
        """per frame: the size of the terms the back-substitution subtracts (|V^-1 g_f| + |V^-1 W^T delta_s|) -- the scale of its rounding"""
        W = self.W32 if (self.w32 if w32 is None else w32) else self.W64
        a = np.linalg.norm(np.einsum("fij,fj->fi", self.Vinv, self.gf), axis=1)
        c = np.linalg.norm(np.einsum("fij,fj->fi", self.Vinv, np.einsum("efj,e->fj", W, ds_)), axis=1)
        return a + c

    def exact_step(self, w32=None):
        """the exact damped step in z order"""
        ds_ = self.solve_s(w32)
        return self.assemble(ds_, self.backsub(ds_, w32))

    def assemble(self, ds_, df):
        d = np.zeros(self.P)
        d[self.ent] = ds_
        d[self.frames] = np.asarray(df).reshape(-1)
        return d

    def split(self, delta):
        """(delta_s, delta_f [F][6]) of a step in z order"""
        delta = np.asarray(delta)
        return delta[self.ent], delta[self.frames].reshape(self.F, 6)

    # ---- certificate quantities ----
    def _pick(self, w32):
        return (self.A32, self.b32) if (self.w32 if w32 is None else w32) else (self.A64, self.b64)

    def residual(self, ds_, w32=None):
        A, b = self._pick(w32)
        return b - A @ ds_

    def rel_residual(self, ds_, w32=None):
        """|b - A delta_s|_2 / |b|_2"""
        A, b = self._pick(w32)
        return np.linalg.norm(b - A @ ds_) / np.linalg.norm(b) if len(b) else 0.0

    def block_jacobi(self, w32=None):
        """inverses of the 6x6 diagonal blocks of A in k_spcg's layout: consecutive 6-chunks of the entity unknowns (a trailing chunk of an
        odd number of intrinsics entities is 3 wide; the padding is identity).  Returns a dense block-diagonal D^-1."""
        A, _ = self._pick(w32)
        n = len(A)
        Dinv = np.zeros((n, n))
        for o in range(0, n, 6):
            s = slice(o, min(o + 6, n))
            Dinv[s, s] = np.linalg.inv(A[s, s])
        return Dinv

    # ---- the absolute-value sums of the direct chain's rounding bound (tests/direct_certificate.py) ----
    def frame_conds(self):
        """cond_2 of every damped frame block V_f [F]: the device inverts V_f, that inverse's error enters with this factor"""
        return np.linalg.cond(self.V) if self.F else np.zeros(0)

    def abs_sums(self):
        """the sums below, computed once per system"""
        if not hasattr(self, "_abs"):
            self._abs = self._abs_sums()
        return self._abs

    def _abs_sums(self):
        """(|U| + sum_f kappa_f |W_f| |V_f^-1| |W_f^T|  [n][n],  |g_s| + sum_f kappa_f |W_f| |V_f^-1| |g_f|  [n]) with fp64 W: what the terms of A
        and b add up to in absolute value, every frame's share weighted with the condition number of the block that is inverted for it"""
        n = len(self.ent)
        if not self.F:
            return np.abs(self.U), np.abs(self.gs)
        Wa = np.abs(self.W64)
        T = np.einsum("efi,fij->efj", Wa, self.frame_conds()[:, None, None] * np.abs(self.Vinv))
        EA = np.abs(self.U) + T.reshape(n, 6 * self.F) @ Wa.reshape(n, 6 * self.F).T
        Eb = np.abs(self.gs) + np.einsum("efj,fj->e", T, np.abs(self.gf))
        return EA, Eb

    def frames_seen(self):
        """per entity unknown: the number of frames whose W block has an entry in its row"""
        return (self.W64 != 0.0).any(axis=2).sum(axis=1) if self.F else np.zeros(len(self.ent), int)

    def energy_norms(self, ds_, w32=None):
        """(r^T D^-1 r, b^T D^-1 b, b^T A^-1 b)"""
        A, b = self._pick(w32)
        r = b - A @ ds_
        Dinv = self.block_jacobi(w32)
        return float(r @ Dinv @ r), float(b @ Dinv @ b), float(b @ self.solve_s(w32))
