"""The constant-velocity sigma fit's model on the CPU: the float64 restatement tests/smooth_cv_fit_restated.py checked against
itself, an exact linear-Gaussian toy and simulated sequences that follow the model.  CPU only.
"""
import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_fit_cases as cc
import smooth_cv_fit_restated as cfr
import smooth_fit_cases as fc
import track_restated as tr

SROT, STRANS, SROT0, STRANS0 = cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0


def _hole(F):
    """frame times with a hole of five at every third pair from pair 1 on (smooth_fit_cases.gaps has its first hole at pair 3)"""
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(F - 1) % 3 == 1) * 4.0])


# ---- 1. U_d: the trace identity against the direct sum ----
@pytest.mark.parametrize("variant", ["plain", "hole", "ends_emptied"])
@pytest.mark.parametrize("F", [3, 4, 17])
def test_the_two_forms_of_the_data_trace_agree(F, variant):
    ds = aar.synth(2, num_frames=F)
    empty = [0, F - 1] if variant == "ends_emptied" else []
    ds = sc.without_frames(ds, empty)
    x0 = sc.track_start(ds)
    ft = _hole(F) if variant == "hole" else None
    td = tr.TrackData(ds, x0)
    assert all(td.start[f + 1] == td.start[f] for f in empty)
    e = cfr.estep(cfr.CvFitProblem(td, SROT0, STRANS0, ft), td.z0, SROT, STRANS, SROT0, STRANS0)
    err = abs(e["U_d_trace"] - e["U_d_direct"]) / abs(e["U_d_direct"])
    share = e["sums"][1] / SROT ** 2 + e["sums"][3] / STRANS ** 2 + e["u_0"]
    print("F %d %s: U_d %.12g (direct %.12g), %.2e; the prior's share %.6g of %d" % (F, variant, e["U_d_trace"], e["U_d_direct"], err, share, 6 * F))
    assert err <= 1e-9, err
    assert 0 < e["U_d_direct"] < 6 * F and 0 < share < 6 * F and np.all(e["terms"][:, [1, 3]] > 0)
    assert e["terms"].shape == (F - 1, 4)


# ---- 2. a linear toy: no M-step decreases the exact marginal likelihood ----
def _toy(seed, F=40, m=2):
    """positions x_f in R^3 whose second differences x_{f+1} - x_f - r_f (x_f - x_{f-1}) have the variance s_t D_f per axis, the first
    difference the variance s_0 D_0, a flat prior on x_0; m direct measurements per frame with variance q; time holes, frames without data"""
    rng = np.random.default_rng(seed)
    dt = np.diff(fc.gaps(F))
    x = np.zeros((F, 3))
    x[1] = rng.normal(size=3) * 0.5 * np.sqrt(dt[0])
    for f in range(1, F - 1):
        x[f + 1] = x[f] + dt[f] / dt[f - 1] * (x[f] - x[f - 1]) + rng.normal(size=3) * 0.3 * np.sqrt(dt[f])
    cnt = np.full(F, m)
    cnt[[5, 6, 20, F - 1]] = 0                      # frames without measurements, the last among them
    ybar = np.stack([x[f] + rng.normal(size=(max(c, 1), 3)).mean(axis=0) * 0.8 if c else np.zeros(3) for f, c in enumerate(cnt)])
    # (the scatter of a frame's measurements about their mean is a constant of the data: part of data_cost at every x)
    scatter = float(sum(rng.chisquare(3 * (c - 1)) * 0.8 ** 2 for c in cnt if c > 1))
    return dt, cnt, ybar, scatter


def _toy_pieces(dt, cnt, ybar, scatter, q, s_t, s_0):
    """the unscaled H (data variance 1) at the effective variances s_t / q and s_0 / q -- s_0 physical and held --, the rows B of the prior's
    errors, the estimate, the data cost and the exact log marginal likelihood (up to a constant of the data)"""
    F = len(cnt)
    B = np.zeros((F - 1, F))
    B[0, :2] = [-1.0, 1.0]
    for f in range(1, F - 1):
        r = dt[f] / dt[f - 1]
        B[f, f - 1:f + 2] = [r, -(1.0 + r), 1.0]
    w = 1.0 / (np.r_[s_0, np.full(F - 2, s_t)] * dt)            # physical weights
    H1 = np.diag(cnt.astype(np.float64)) + q * (B.T * w) @ B    # per axis; the three axes are independent copies
    xh = np.linalg.solve(H1, cnt[:, None] * ybar)
    data = float(np.sum(cnt[:, None] * (ybar - xh) ** 2)) + scatter
    e = B @ xh
    prior = float(np.sum(w[:, None] * e * e))
    n_y = 3 * int(cnt.sum())
    _, logdet = np.linalg.slogdet(H1 / q)
    loglik = -0.5 * n_y * np.log(2 * np.pi * q) + 1.5 * np.sum(np.log(w)) - 1.5 * logdet - 0.5 * (data / q + prior)
    return H1, B, xh, data, float(loglik), n_y


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_no_m_step_decreases_the_exact_marginal_likelihood(seed):
    dt, cnt, ybar, scatter = _toy(seed)
    F = len(cnt)
    q, s_t, s_0 = 1.0, 0.05 ** 2, 0.5 ** 2
    last = None
    for it in range(25):
        H1, B, xh, data, loglik, n_y = _toy_pieces(dt, cnt, ybar, scatter, q, s_t, s_0)
        if last is not None:
            assert loglik >= last - 1e-9 * abs(last), (it, loglik, last)
        last = loglik
        S = np.linalg.inv(H1)
        e = B @ xh
        a = np.sum(e * e, axis=1) / dt
        u = 3.0 * np.einsum("fi,ij,fj->f", B, S, B) / dt
        A_t, U_t = float(np.sum(a[1:])), float(np.sum(u[1:]))               # the terms 1 .. F-2 only
        u_0 = float(u[0] / (s_0 / q))
        U_d = 3.0 * F - U_t / (s_t / q) - u_0                               # tr(H H^-1) = 3 F here: three unknowns per frame
        assert abs(U_d - 3.0 * float(np.sum(cnt * np.diag(S)))) <= 1e-8 * F
        q, _, s_t = cfr.mstep([0.0, 0.0, A_t, U_t], data, U_d, q, 1.0, s_t, F, n_y / 8.0, estimate=(1, 0, 1))
    print("seed %d: sigma_px %.4f (0.8), sigma_trans %.4f (0.3), log likelihood %.6f" % (seed, np.sqrt(q), np.sqrt(s_t), last))


# ---- 3. recovery ----
def test_the_recovery_sequence_meets_its_conditions():
    ds, x0 = cc.cv_walk(cc.CV_SEEDS[0])
    rot, trans, ratio = cc.recovery_conditions(ds, x0)
    eff = np.array([1.0, SROT, STRANS]) / np.array([cc.CV_SIGMAS[0], cc.CV_SIGMAS[1] / cc.CV_SIGMAS[0], cc.CV_SIGMAS[2] / cc.CV_SIGMAS[0]])
    print("drift %.3f rad %.3f m, smallest sigma / pose std %.3f, start values off by %s" % (rot, trans, ratio, np.array2string(eff, precision=2)))
    assert rot <= 0.5 and trans <= 0.3                 # 1.
    assert ratio >= 0.3                                # 2.
    assert np.all(np.maximum(eff, 1.0 / eff) >= 3.0)   # 3.
    assert max(cc.CAPS) <= 0.25 and ds.num_frames <= 400   # 4.


@pytest.mark.parametrize("seed", cc.CV_SEEDS)
def test_recovery_of_a_simulated_constant_velocity_sequence(seed):
    ds, x0 = cc.cv_walk(seed)
    td = tr.TrackData(ds, x0)
    r = cfr.fit(cfr.CvFitProblem(td, SROT0, STRANS0), td.z0, SROT, STRANS, max_iters=cc.CV_MAX_ITERS)
    dev = np.array([r["sigma_px"], r["sigma_rot"], r["sigma_trans"]]) / cc.CV_SIGMAS - 1.0
    print("seed %d: %d EM iterations (exit %d), deviations %s, caps %s" % (seed, r["iterations"], r["stop_code"], np.array2string(dev, precision=5),
                                                                          np.array2string(np.array(cc.CAPS), precision=5)))
    assert r["stop_code"] == 1
    assert np.all(np.abs(dev) <= cc.CAPS), (dev, cc.CAPS)
