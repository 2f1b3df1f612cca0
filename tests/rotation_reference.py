"""Multiprecision reference of the pose-difference terms -- TEST INFRASTRUCTURE ONLY (mpmath).

Every term that compares two poses -- the pose priors (csrc/prior_kernels.hip), the relative pose priors (csrc/pair_prior_kernels.hip), the
between factor of the smoothed and the live tracker (csrc/pair_terms.hpp) -- is the logarithm of a product of rotations plus a translation
difference.  This module states the three residuals FROM THEIR DEFINITIONS and differentiates them numerically, in mpmath:

    exp          R = I + sin(t)/t [w]x + (1 - cos t)/t^2 [w]x^2, t = |w|
    log          phi = atan2(|v|/2, c) / |v| v,  v = vee(Q - Q^T), c = (tr Q - 1)/2; at exactly pi (v = 0, c = -1) the axis comes from the
                 symmetric part (Q + I)/2 = n n^T and either sign is a valid answer (the one with a positive leading component is returned)
    pose prior   e = [log(R_p^T R) ; t - t_p]                                              (include/aar.h, prior_kernels.hip)
    relative     e = [log(R_rel^T R_a^T R_b) ; R_a^T (t_b - t_a) - t_rel]                  
    between      e = [log((R_a dR)^T R_b) ; t_b - t_a - dt]                                (DESIGN.md sections 15, 16, 25)
    Jacobian     central differences over the 6 or 12 pose entries, step 1e-20.  No analytic derivation, no J_l, no J_r^-1.
    terms        J^T L J, -J^T L e, e^T L e in mp, rounded to float64 at the very end

and every quantity is evaluated AT THE FLOAT64 INPUTS (converted exactly), not at the angle a case was meant to have.

Precision.  The design asks for 50 digits.  The logarithm's error is eps_mp / sin(theta): one part in 1e34 at the closest a float64 rotation
vector comes to a half turn (pi - fl(pi) = 1.2e-16).  A central difference with step 1e-20 divides that by 2e-20, which would leave 1e-14 in J --
more than the error it is meant to measure.  So the context below works at 60 digits: 1e-24 in J at that case, at most 1e-38 elsewhere; the
truncation error of the difference, h^2 f''' / 6, is 1e-40 times a third derivative of order one (the logarithm is analytic inside the ball of
radius pi, and no case sits closer to its surface than 1e-16 >> h).  The context is private: mpmath.mp itself is not touched.

The second part of the module evaluates THE SAME QUANTITIES in float64 numpy, mp-free, by the textbook closed forms in their stable variants.
It is there to be compared with the mp values (tests/test_rotation_reference_host.py): the error of a careful float64 evaluation is the unit in
which the bars of the GPU tests are stated.  It shares no code with csrc/ or with the restatements reduced_system / smooth_restated.
"""
import mpmath
import numpy as np

DPS = 60
STEP = "1e-20"
M = mpmath.mp.clone()
M.dps = DPS
_h = M.mpf(STEP)
_0, _1, _2 = M.mpf(0), M.mpf(1), M.mpf(2)


# ---------------------------------------------------------------- mp: rotations
def mpv(x):
    """a float64 array-like as a list of mp numbers, exactly"""
    return [v if isinstance(v, M.mpf) else M.mpf(float(v)) for v in x]


def mat_mul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def mat_t(A):
    return [[A[j][i] for j in range(3)] for i in range(3)]


def mat_vec(A, x):
    return [A[i][0] * x[0] + A[i][1] * x[1] + A[i][2] * x[2] for i in range(3)]


_exp_cache = {}


def exp(w):
    """the rotation matrix of the rotation vector w (3 mp numbers)"""
    key = (w[0], w[1], w[2])
    R = _exp_cache.get(key)
    if R is not None:
        return R
    x, y, z = key
    t2 = x * x + y * y + z * z
    if t2 == 0:
        R = [[_1, _0, _0], [_0, _1, _0], [_0, _0, _1]]
    else:
        t = M.sqrt(t2)
        a, b = M.sin(t) / t, (_1 - M.cos(t)) / t2
        R = [[_1 - b * (y * y + z * z), -a * z + b * x * y, a * y + b * x * z],
             [a * z + b * x * y, _1 - b * (x * x + z * z), -a * x + b * y * z],
             [-a * y + b * x * z, a * x + b * y * z, _1 - b * (x * x + y * y)]]
    if len(_exp_cache) > 200000:
        _exp_cache.clear()
    _exp_cache[key] = R
    return R


def log(Q):
    """the rotation vector (3 mp numbers, angle in [0, pi]) of the rotation matrix Q"""
    v = [Q[2][1] - Q[1][2], Q[0][2] - Q[2][0], Q[1][0] - Q[0][1]]
    n = M.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = (Q[0][0] + Q[1][1] + Q[2][2] - _1) / _2
    if n == 0:
        if c > 0:
            return [_0, _0, _0]
        # exactly a half turn: (Q + I)/2 = n n^T; the largest diagonal entry gives the pivot, both signs are valid
        S = [[(Q[i][j] + (_1 if i == j else _0)) / _2 for j in range(3)] for i in range(3)]
        p = max(range(3), key=lambda i: S[i][i])
        d = M.sqrt(S[p][p])
        return [M.pi * S[p][j] / d for j in range(3)]
    k = M.atan2(n / _2, c) / n
    return [k * v[0], k * v[1], k * v[2]]


def angle(phi):
    return M.sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2])


_rot_cache = {}


def rot_residual(w_ref, w_a, w_b):
    """log(Exp(w_ref)^T Exp(w_a)^T Exp(w_b)): the rotation part of all three residuals (w_a = 0 for the pose prior)"""
    key = (w_ref[0], w_ref[1], w_ref[2], w_a[0], w_a[1], w_a[2], w_b[0], w_b[1], w_b[2])
    phi = _rot_cache.get(key)
    if phi is None:
        phi = log(mat_mul(mat_t(exp(w_ref)), mat_mul(mat_t(exp(w_a)), exp(w_b))))
        if len(_rot_cache) > 200000:
            _rot_cache.clear()
        _rot_cache[key] = phi
    return phi


# ---------------------------------------------------------------- mp: the three residuals, from their definitions
def prior_e(x6, xp):
    """[log(R_p^T R) ; t - t_p]"""
    return rot_residual(xp[:3], [_0, _0, _0], x6[:3]) + [x6[3 + i] - xp[3 + i] for i in range(3)]


def pair_e(xa, xb, xrel):
    """[log(R_rel^T R_a^T R_b) ; R_a^T (t_b - t_a) - t_rel]"""
    d = mat_vec(mat_t(exp(xa[:3])), [xb[3 + i] - xa[3 + i] for i in range(3)])
    return rot_residual(xrel[:3], xa[:3], xb[:3]) + [d[i] - xrel[3 + i] for i in range(3)]


def between_e(za, zb, rel=None):
    """[log((R_a dR)^T R_b) ; t_b - t_a - dt], (dR, dt) = rel or the identity"""
    if rel is None:
        rel = [_0] * 6
    return rot_residual(rel[:3], za[:3], zb[:3]) + [zb[3 + i] - za[3 + i] - rel[3 + i] for i in range(3)]


def jacobian(fun, xs, consts=()):
    """d fun(*xs, *consts) / d (the entries of every vector of xs, in order) by central differences with step 1e-20: rows x columns as lists"""
    cols = []
    for n, x in enumerate(xs):
        for k in range(len(x)):
            hi, lo = list(x), list(x)
            hi[k] = x[k] + _h
            lo[k] = x[k] - _h
            fp = fun(*(list(xs[:n]) + [hi] + list(xs[n + 1:]) + list(consts)))
            fm = fun(*(list(xs[:n]) + [lo] + list(xs[n + 1:]) + list(consts)))
            cols.append([(a - b) / (_2 * _h) for a, b in zip(fp, fm)])
    return [[c[r] for c in cols] for r in range(len(cols[0]))]


class Terms:
    """e [6], J [6, 6 n], H = J^T L J [6 n, 6 n], B = -J^T L e [6 n], cost = e^T L e of one term, float64 (rounded from mp at the end)"""

    def __init__(self, e, J, info):
        L = [[M.mpf(float(v)) for v in row] for row in np.asarray(info, dtype=np.float64).reshape(6, 6)]
        n = len(J[0])
        LJ = [[sum(L[r][k] * J[k][c] for k in range(6)) for c in range(n)] for r in range(6)]
        Le = [sum(L[r][k] * e[k] for k in range(6)) for r in range(6)]
        self.e = np.array([float(v) for v in e])
        self.J = np.array([[float(v) for v in row] for row in J])
        up = {(i, j): sum(J[k][i] * LJ[k][j] for k in range(6)) for i in range(n) for j in range(i, n)}      # (L is symmetric: so is J^T L J)
        self.H_mp = [[up[min(i, j), max(i, j)] for j in range(n)] for i in range(n)]      # (kept in mp for sums over terms)
        self.B_mp = [-sum(J[k][i] * Le[k] for k in range(6)) for i in range(n)]
        self.cost_mp = sum(e[k] * Le[k] for k in range(6))
        self.H = np.array([[float(v) for v in row] for row in self.H_mp])
        self.B = np.array([float(v) for v in self.B_mp])
        self.cost = float(self.cost_mp)
        self.angle_mp = angle(e[:3])
        self.angle = float(self.angle_mp)


def prior_terms(x6, xp, info):
    x6, xp = mpv(x6), mpv(xp)
    return Terms(prior_e(x6, xp), jacobian(prior_e, [x6], [xp]), info)


def pair_terms(xa, xb, xrel, info):
    xa, xb, xrel = mpv(xa), mpv(xb), mpv(xrel)
    return Terms(pair_e(xa, xb, xrel), jacobian(pair_e, [xa, xb], [xrel]), info)


def between_terms(za, zb, rel, info):
    za, zb = mpv(za), mpv(zb)
    rel = None if rel is None else mpv(rel)
    return Terms(between_e(za, zb, rel), jacobian(between_e, [za, zb], [rel]), info)


def partner_vector(w, theta, axis, side="ref"):
    """The float64 rotation vector that leaves a residual rotation Exp(theta n) against w, built in mp and rounded once:
    side="ref": w_ref = log(R(w) Exp(theta n)^T), so that R_ref^T R(w) = Exp(theta n)  (the prior's vector of an entity at w; with R(w) = R_ab the
                relative prior's, and the motion log(R_ab Exp(-theta n)) of a between factor);
    side="own": w' = log(R(w) Exp(theta n)), so that R(w)^T R(w') = Exp(theta n)       (the entity's vector against a prior at w)."""
    n = np.asarray(axis, dtype=np.float64)
    tn = [M.mpf(float(theta)) * M.mpf(float(a)) / M.sqrt(sum(M.mpf(float(b)) ** 2 for b in n)) for a in n]
    E = exp(tn)
    R = w if isinstance(w[0], list) else exp(mpv(w))      # (a rotation matrix in mp is taken as it is)
    Q = mat_mul(R, mat_t(E)) if side == "ref" else mat_mul(R, E)
    return np.array([float(v) for v in log(Q)])


def to_numpy(R):
    return np.array([[float(v) for v in row] for row in R])


# ---------------------------------------------------------------- float64: the same quantities by the stable closed forms, mp-free
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _series(coef, t2):
    s = 0.0
    for c in coef[::-1]:
        s = s * t2 + c
    return s


# (t - sin t)/t^3 = sum_k (-1)^k t^(2k) / (2k + 3)!  and  (1 - (t/2) cot(t/2))/t^2 = sum_n |B_2n| t^(2n - 2) / (2n)!  below t = 1, where the
# closed forms cancel; the coefficients are exact rationals rounded once
_C_SIN = [float((-1) ** k / mpmath.factorial(2 * k + 3)) for k in range(10)]
_C_COT = [float(abs(mpmath.bernoulli(2 * n)) / mpmath.factorial(2 * n)) for n in range(1, 14)]


def exp64(w):
    w = np.asarray(w, dtype=np.float64)
    t = float(np.sqrt(w @ w))
    if t == 0.0:
        return np.eye(3)
    K = hat(w)
    sh = np.sin(0.5 * t)
    return np.eye(3) + (np.sin(t) / t) * K + (2.0 * sh * sh / (t * t)) * (K @ K)


def log64(Q):
    """atan2 logarithm; beyond pi - 0.1 (sin < 0.1) the axis comes from the symmetric part, its sign from the antisymmetric one"""
    v = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    s = 0.5 * float(np.sqrt(v @ v))
    c = 0.5 * (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1.0)
    t = float(np.arctan2(s, c))
    if s == 0.0 and c > 0:
        return 0.5 * v
    if c > 0 or s >= 0.1:
        return (t / (2.0 * s)) * v
    S = 0.5 * (Q + Q.T) - c * np.eye(3)          # (1 - c) n n^T
    p = int(np.argmax(np.diag(S)))
    n = S[p] / np.linalg.norm(S[p])
    if n @ v < 0:
        n = -n
    return t * n


def jl64(w):
    w = np.asarray(w, dtype=np.float64)
    t2 = float(w @ w)
    t = np.sqrt(t2)
    K = hat(w)
    if t == 0.0:
        return np.eye(3)
    sh = np.sin(0.5 * t)
    b = 2.0 * sh * sh / t2
    c = _series(_C_SIN, t2) if t < 1.0 else (t - np.sin(t)) / (t2 * t)
    return np.eye(3) + b * K + c * (K @ K)


def jrinv64(phi):
    phi = np.asarray(phi, dtype=np.float64)
    t2 = float(phi @ phi)
    t = np.sqrt(t2)
    K = hat(phi)
    k = _series(_C_COT, t2) if t < 1.0 else (1.0 - 0.5 * t * np.cos(0.5 * t) / np.sin(0.5 * t)) / t2
    return np.eye(3) + 0.5 * K + k * (K @ K)


class Terms64:
    def __init__(self, e, J, info):
        L = np.asarray(info, dtype=np.float64).reshape(6, 6)
        self.e, self.J = e, J
        self.H, self.B, self.cost = J.T @ L @ J, -J.T @ L @ e, float(e @ L @ e)


def prior_terms64(x6, xp, info):
    x6, xp = np.asarray(x6, dtype=np.float64), np.asarray(xp, dtype=np.float64)
    phi = log64(exp64(xp[:3]).T @ exp64(x6[:3]))
    J = np.eye(6)
    J[:3, :3] = jrinv64(phi) @ jl64(x6[:3]).T
    return Terms64(np.r_[phi, x6[3:] - xp[3:]], J, info)


def pair_terms64(xa, xb, xrel, info, between=False):
    """the relative prior's terms; between=True: the between factor's (xrel = the expected motion or None)"""
    xa, xb = np.asarray(xa, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    xrel = np.zeros(6) if xrel is None else np.asarray(xrel, dtype=np.float64)
    Ra, Rb = exp64(xa[:3]), exp64(xb[:3])
    phi = log64(exp64(xrel[:3]).T @ (Ra.T @ Rb))
    Ji = jrinv64(phi) @ Rb.T
    J = np.zeros((6, 12))
    J[:3, 0:3] = -Ji @ jl64(xa[:3])
    J[:3, 6:9] = Ji @ jl64(xb[:3])
    d = xb[3:] - xa[3:]
    if between:
        et = d - xrel[3:]
        J[3:, 3:6], J[3:, 9:12] = -np.eye(3), np.eye(3)
    else:
        et = Ra.T @ d - xrel[3:]
        J[3:, 0:3] = Ra.T @ hat(d) @ jl64(xa[:3])
        J[3:, 3:6], J[3:, 9:12] = -Ra.T, Ra.T
    return Terms64(np.r_[phi, et], J, info)


# ---------------------------------------------------------------- the measure
def distances(got_e, got_H, got_B, got_cost, ref):
    """(e: max abs; H: max |dH_ij| / sqrt(H_ii H_jj), the measure of projection_reference.scaled_error; B: max |dB_i| / sqrt(H_ii cost), the same
    scaling (|B_i| <= sqrt(H_ii cost) by Cauchy-Schwarz); cost: relative) of a term against its reference (a Terms)"""
    d = np.sqrt(np.abs(np.diag(ref.H)))
    de = float(np.abs(np.asarray(got_e) - ref.e).max())
    dH = float((np.abs(np.asarray(got_H) - ref.H) / np.outer(d, d)).max())
    dB = float((np.abs(np.asarray(got_B) - ref.B) / (d * np.sqrt(ref.cost))).max())
    dc = abs(got_cost - ref.cost) / ref.cost
    return de, dH, dB, dc


def assemble_chain(terms):
    """(diag [F, 6, 6], off [F - 1, 6, 6], rhs [6 F], cost) of a chain of between factors, pair f = (frame f, frame f + 1): the blocks summed in mp
    and rounded once, in the layout of Problem.track_smooth_system"""
    F = len(terms) + 1
    diag = [[[_0] * 6 for _ in range(6)] for _ in range(F)]
    rhs = [[_0] * 6 for _ in range(F)]
    off = np.zeros((F - 1, 6, 6))
    cost = _0
    for f, t in enumerate(terms):
        for i in range(6):
            for j in range(6):
                diag[f][i][j] += t.H_mp[i][j]
                diag[f + 1][i][j] += t.H_mp[6 + i][6 + j]
                off[f, i, j] = float(t.H_mp[i][6 + j])
            rhs[f][i] += t.B_mp[i]
            rhs[f + 1][i] += t.B_mp[6 + i]
        cost += t.cost_mp
    return (np.array([[[float(v) for v in r] for r in b] for b in diag]), off, np.array([[float(v) for v in r] for r in rhs]).reshape(-1), float(cost))


def chain_distances(gd, go, gr, ref_diag, ref_off, ref_rhs, pair_cost):
    """per pair f: (H, B) distances of the blocks pair f touches -- diag[f], diag[f + 1], off[f] in the scaled measure |dH_ij| / sqrt(H_ii H_jj), and
    rhs of the two frames as |dB_i| / sqrt(H_ii (sum of the costs of the pairs at that frame))"""
    F = len(ref_diag)
    d = np.sqrt(np.abs(np.einsum("fii->fi", ref_diag)))
    eD = np.array([(np.abs(gd[f] - ref_diag[f]) / np.outer(d[f], d[f])).max() for f in range(F)])
    eO = np.array([(np.abs(go[f] - ref_off[f]) / np.outer(d[f], d[f + 1])).max() for f in range(F - 1)])
    c = np.r_[0.0, pair_cost] + np.r_[pair_cost, 0.0]
    eB = (np.abs(gr - ref_rhs).reshape(F, 6) / (d * np.sqrt(c)[:, None])).max(axis=1)
    return np.maximum(np.maximum(eD[:-1], eD[1:]), eO), np.maximum(eB[:-1], eB[1:])
