"""Float64 restatement of aar_problem_detection_loo / aar_problem_gate_detections -- TEST INFRASTRUCTURE ONLY, numpy only (DESIGN.md
section 37).  It stands on tests/predict_restated.py's PredictSystem (the column bookkeeping, the mask rule) and the complex-step J of
tests/projection_reference.py.

The tail (`tail`): what the kernel does behind C_i -- A = I - C (mode 3) or I + C (mode 4), its Cholesky factor without pivoting, A w = r,
q = r^T w, k = w^T C w, margin = the smallest pivot met, UNDETERMINED where a pivot is <= MIN_PIVOT or not finite -- and `statistics`: F
and Cook's distance from q, k and the call's scalars.  `fault` plants the mistakes such a tail can make:

    "c_sign"     the sign of C flipped in mode 3 (A = I + C)
    "c_diag"     diag(C) used for C
    "cook_sign"  r taken with the opposite sign inside Cook's distance only (k = w(-r)^T C w(r) = -k)
    "nu"         nu used where nu - 8 belongs

The linear problem (LooSystem): the dense J (8 N x P_live, complex step) and r = observed - u at x, the priors' H_p as a quadratic term,

    cost(d) = |r - J d|^2 + d^T H_p d,      H = J^T J + H_p,      d^ = H^-1 J^T r,      rho = r - J d^  (the residual AT the linear minimum).

Every identity the statistic rests on is EXACT for this problem and is checked by a route that never forms (I - C_i)^-1: with
H_(i) = H - J_i^T J_i solved densely by numpy (`deleted`),

    (I - C_i)^-1 rho_i = rho_i + J_i H_(i)^-1 J_i^T rho_i                       (Woodbury)
    q_i = rho_i^T (I - C_i)^-1 rho_i = min cost - min cost without detection i's rows
    I + C_(i) = (I - C_i)^-1,   C_(i) = J_i H_(i)^-1 J_i^T                    (the gate of the reduced system)
    k_i = (d^ - d^_(i))^T H (d^ - d^_(i))                                      (Cook's distance by the moved solution)
    F_i = (q_i / 8) / (min cost without i / (nu - 8))
"""
import numpy as np

import predict_restated as prs

MIN_PIVOT = 1e-6          # PREDICT_LOO_MIN_PIVOT of csrc/kernels.h
UNDETERMINED = 4
FAULTS = ("c_sign", "c_diag", "cook_sign", "nu")
U53 = 2.0 ** -53


def tail(C, r, mode=3, fault=None):
    """(w [8], q, k, margin, undetermined) of one query: the kernel's tail on C (8 x 8) and r (8)"""
    C = np.asarray(C, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    Cu = np.diag(np.diag(C)) if fault == "c_diag" else C
    A = np.eye(8) + Cu if (mode == 4 or fault == "c_sign") else np.eye(8) - Cu
    L = np.zeros((8, 8))
    A = A.copy()
    margin = np.inf
    for k in range(8):
        d = A[k, k]
        if not d >= margin:
            margin = d
        if not d > MIN_PIVOT or not np.isfinite(d):
            return np.full(8, np.nan), np.nan, np.nan, margin, True
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = A[k + 1:, k] / L[k, k]
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    y = np.zeros(8)
    for i in range(8):
        y[i] = (r[i] - L[i, :i] @ y[:i]) / L[i, i]
    w = np.zeros(8)
    for i in range(7, -1, -1):
        w[i] = (y[i] - L[i + 1:, i] @ w[i + 1:]) / L[i, i]
    q = float(r @ w)
    k = float(w @ (Cu @ w))
    if fault == "cook_sign":
        k = -k
    return w, q, k, margin, False


def tails(C, r, mode=3, fault=None):
    """`tail` over arrays C [n, 8, 8], r [n, 8]; rows whose C is NaN (status bits 0, 1) give NaN and undetermined = False"""
    n = len(C)
    w, q, k, mg, und = np.full((n, 8), np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, dtype=bool)
    for i in range(n):
        if np.isfinite(C[i]).all():
            w[i], q[i], k[i], mg[i], und[i] = tail(C[i], r[i], mode, fault)
    return w, q, k, mg, und


def statistics(q, k, sum_sq, nu, num_live_vars, fault=None):
    """(F, cook) as the kernel forms them from q, k and the call's scalars (sigma2 = sum_sq / nu)"""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    dof = nu if fault == "nu" else nu - 8
    F = np.full(q.shape, np.nan)
    if nu > 8:
        with np.errstate(divide="ignore", invalid="ignore"):
            den = (sum_sq - q) / float(dof)
            F = np.where(np.isnan(q), np.nan, np.where(den <= 0.0, np.inf, (q / 8.0) / den))
    sigma2 = sum_sq / float(nu) if nu > 0 else np.nan
    return F, k / (float(num_live_vars) * sigma2)


def solve_bar(C, mode=3):
    """64 eps kappa_2(A): the operation count of an 8 x 8 factor and two substitutions in the project's eps-kappa style (eps = 2^-53)"""
    A = np.eye(8) - C if mode == 3 else np.eye(8) + C
    return 64.0 * U53 * np.linalg.cond(0.5 * (A + A.T))


class LooSystem:
    """The linear problem of a PredictSystem at x: dense J over the live columns, r = observed - u, H = J^T J + H_p."""

    def __init__(self, ps, x, obs_uv=None, Hp=None):
        ds = ps.ds
        self.ps, self.x = ps, np.asarray(x, dtype=np.float64)
        self.q3 = prs.detection_queries(ds)
        uv, J18, depth = prs.query_projection(ds, self.x, self.q3)
        assert (depth > 0).all()
        obs = np.asarray(ds.obs_uv if obs_uv is None else obs_uv, dtype=np.float32).reshape(-1, 8).astype(np.float64)
        self.N, self.P = len(self.q3), ps.num_live_vars
        self.uv = uv
        self.r = obs - uv
        self.cols = np.full((self.N, 18), -1, dtype=np.int64)       # position in the live unknowns of each of the 18 parameters, or -1
        for i, (c, m, f) in enumerate(self.q3):
            z = ps.z_columns(int(c), int(m), int(f))
            self.cols[i] = [ps.pos.get(int(v), -1) if v >= 0 else -1 for v in z]
        self.J18 = np.where(self.cols[:, None, :] >= 0, J18, 0.0)
        self.Hp = np.zeros((self.P, self.P)) if Hp is None else np.asarray(Hp, dtype=np.float64)[np.ix_(ps.idx, ps.idx)]
        H = self.Hp.copy()
        g = np.zeros(self.P)
        for i in range(self.N):
            ok = self.cols[i] >= 0
            p = self.cols[i][ok]
            Ji = self.J18[i][:, ok]
            H[np.ix_(p, p)] += Ji.T @ Ji
            g[p] += Ji.T @ self.r[i]
        self.H, self.g = H, g
        self.Hinv = np.linalg.inv(H)
        self.delta = self.Hinv @ g
        self.rho = self.r - self.times(self.delta)
        self.cost_min = float((self.rho ** 2).sum() + self.delta @ self.Hp @ self.delta)

    def times(self, d):
        """J d for every detection: [N, 8]"""
        dx = np.where(self.cols >= 0, d[np.maximum(self.cols, 0)], 0.0)
        return np.einsum("nrk,nk->nr", self.J18, dx)

    def abs_times(self, d):
        """|J| d for every detection: [N, 8]"""
        dx = np.where(self.cols >= 0, d[np.maximum(self.cols, 0)], 0.0)
        return np.einsum("nrk,nk->nr", np.abs(self.J18), dx)

    def row(self, i):
        """J_i (8 x P_live), dense"""
        J = np.zeros((8, self.P))
        ok = self.cols[i] >= 0
        J[:, self.cols[i][ok]] = self.J18[i][:, ok]
        return J

    def C(self, i):
        ok = self.cols[i] >= 0
        p = self.cols[i][ok]
        Ji = self.J18[i][:, ok]
        return Ji @ self.Hinv[np.ix_(p, p)] @ Ji.T

    def all_C(self):
        return np.stack([self.C(i) for i in range(self.N)])

    def deleted(self, i):
        """The problem without detection i, solved densely: (C_(i) = J_i H_(i)^-1 J_i^T, w = rho_i + C_(i) rho_i, the drop of the minimal cost,
        the minimal cost without i, k = (d^ - d^_(i))^T H (d^ - d^_(i)))"""
        Ji = self.row(i)
        Hd = self.H - Ji.T @ Ji
        gd = self.g - Ji.T @ self.r[i]
        X = np.linalg.solve(Hd, np.column_stack([Ji.T, gd]))
        Cd = Ji @ X[:, :8]
        dd = X[:, 8]
        # min over d of sum_{j != i} |r_j - J_j d|^2 + d^T H_p d, written out at d^_(i) (no normal-equation shortcut: the sum itself)
        rd = self.r - self.times(dd)
        rd[i] = 0.0
        cost_d = float((rd ** 2).sum() + dd @ self.Hp @ dd)
        move = self.delta - dd
        return Cd, self.rho[i] + Cd @ self.rho[i], self.cost_min - cost_d, cost_d, float(move @ self.H @ move)


def gauss_newton(ds, obs_uv, x0, iters=30, tol=1e-12):
    """Float64 Gauss-Newton on every unknown of an all-optimised problem without priors (dense J, complex step), from x0 to convergence:
    (x, the step norms).  The additive chart of x_full: z column = x_full index."""
    x = np.asarray(x0, dtype=np.float64).copy()
    steps = []
    for _ in range(iters):
        ls = system_at(ds, x, obs_uv)        # (the oracle's H only tells the PredictSystem which rows are live; LooSystem builds its own)
        dz = np.zeros(len(x))
        dz[ls.ps.idx] = ls.delta
        x = x + dz
        steps.append(float(np.linalg.norm(dz)))
        if steps[-1] <= tol * max(1.0, float(np.linalg.norm(x))):
            break
    return x, steps


# ---- the planted outlier (tests/test_loo_restated_host.py (d), tests/test_gpu_detection_loo.py 5): a synthetic set with pixel noise in which
# one detection has few others to contradict it -- marker PLANT_MARKER keeps its first two detections and the frame of the first of them keeps
# four -- so that a shift of that detection's corners is mostly absorbed by its marker's and its frame's pose
PLANT_SYNTH = dict(num_cams=4, num_markers=8, num_frames=30, noise_px=0.5, seed=2, min_view_cos=0.05)
PLANT_MARKER, PLANT_MARKER_KEEPS, PLANT_FRAME_KEEPS = 3, 2, 4
PLANT_OFFSET = (6.0, -4.0)        # pixels, added to (u, v) of each of the four corners
PLANT_LEVERAGE_BELOW = 6.0
PLANT_F_MAX = 3.27                # the 0.999 quantile of F(8, nu - 8) for large nu: chi2_8(0.999) / 8 = 26.12 / 8


def planted_base():
    """the cut synthetic set, no outlier planted yet"""
    import aar
    ds0 = aar.synth(2, **PLANT_SYNTH)
    fr, mk = np.asarray(ds0.obs_frame), np.asarray(ds0.obs_marker)
    keep = np.ones(ds0.num_obs, dtype=np.uint8)
    im = np.nonzero(mk == PLANT_MARKER)[0]
    keep[im[PLANT_MARKER_KEEPS:]] = 0
    others = np.nonzero((fr == fr[im[0]]) & (mk != PLANT_MARKER))[0]
    keep[others[PLANT_FRAME_KEEPS - 1:]] = 0
    return ds0.select_observations(keep)


def with_corners(ds, obs_uv):
    """a copy of ds with other observed corners"""
    out = type(ds).__new__(type(ds))
    out.__dict__.update(ds.__dict__)
    out.obs_uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 8)
    return out


def plant_index(leverage):
    """THE RULE: the detection with the highest leverage below PLANT_LEVERAGE_BELOW (the first of them on a tie)"""
    lev = np.asarray(leverage, dtype=np.float64)
    return int(np.argmax(np.where(lev < PLANT_LEVERAGE_BELOW, lev, -np.inf)))


def plant(ds, i):
    """(the set with detection i shifted by PLANT_OFFSET, the shift [8])"""
    shift = np.tile(np.asarray(PLANT_OFFSET, dtype=np.float32), 4)
    obs = np.asarray(ds.obs_uv, dtype=np.float32).reshape(-1, 8).copy()
    obs[i] += shift
    return with_corners(ds, obs), shift.astype(np.float64)


def system_at(ds, x, obs_uv=None):
    """LooSystem of an all-optimised problem without priors at x"""
    import oracle_lib as ol
    H0, _ = ol.Oracle(ds).normal_equations(np.asarray(x, dtype=np.float64), res_mode=ol.RES_F64)
    return LooSystem(prs.PredictSystem(ds, H0), x, obs_uv)
# |w - (shift + clean residual)|_inf of the planted detection in the restatement: MEASURED 1.590187 px (test_loo_restated_host.py (d)); the
# constant is that figure rounded up in its fifth digit
PLANT_GAP = 1.5902


# ---- the second-order gap of the linearisation (tests/test_loo_restated_host.py (e), tests/test_gpu_detection_loo.py 6)
# MEASURED on sweep2 (test_loo_restated_host.py (e)): |innovation - w|_inf 9.4e-6, 2.6e-5, 1.5e-5 px and |drop - q| / q 1.9e-6, 7.4e-6,
# 7.1e-6 for the three detections; the constants are the worst of each (2.625e-5, 7.436e-6), rounded up in the third digit
GAP_W = 2.63e-5                   # pixels
GAP_Q = 7.44e-6                   # relative to q


def three_detections(leverage, q):
    """the detections of the deletion tests: the highest leverage, the median leverage, the largest q"""
    lev = np.asarray(leverage, dtype=np.float64)
    out = [int(np.argmax(lev)), int(np.argsort(lev)[len(lev) // 2]), int(np.nanargmax(q))]
    assert len(set(out)) == 3
    return out
