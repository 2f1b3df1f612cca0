"""The sigma fit's model on the CPU: the float64 restatement tests/smooth_fit_restated.py checked against itself, an exact
linear-Gaussian toy and simulated random walks; the host side of aar_smooth_fit_params.  CPU only.
"""
import ctypes as C

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_fit_cases as fc
import smooth_fit_restated as fr
import track_restated as tr

SROT, STRANS = fc.SROT, fc.STRANS


# ---- 1. U_d: the trace identity against the direct sum ----
@pytest.mark.parametrize("variant", ["plain", "gaps", "rel", "gaps_rel"])
@pytest.mark.parametrize("F", [2, 3, 17])
def test_the_two_forms_of_the_data_trace_agree(F, variant):
    ds = aar.synth(2, num_frames=F)
    empty = [0, F - 1] if F == 17 else []          # (smooth_cases.emptied starts at 30 frames; its choice of the two ends here)
    ds = sc.without_frames(ds, empty)
    x0 = sc.track_start(ds)
    ft = fc.gaps(F) if "gaps" in variant else None
    rel = fc.rel_motion(F) if "rel" in variant else None
    td = tr.TrackData(ds, x0)
    assert all(td.start[f + 1] == td.start[f] for f in empty)
    e = fr.estep(fr.FitProblem(td, ft, rel), td.z0, SROT, STRANS)
    err = abs(e["U_d_trace"] - e["U_d_direct"]) / abs(e["U_d_direct"])
    print("F %d %s: U_d %.12g (direct %.12g), %.2e" % (F, variant, e["U_d_trace"], e["U_d_direct"], err))
    assert err <= 1e-9, err
    assert 0 < e["U_d_direct"] < 6 * F and np.all(e["terms"] > 0)


# ---- 2. a linear toy: no M-step decreases the exact marginal likelihood ----
def _toy(seed, F=40, m=2):
    """positions x_f in R^3 on a random walk (variance s_t D_f per axis, a flat prior on x_0), m direct measurements per frame with variance q"""
    rng = np.random.default_rng(seed)
    dt = np.diff(fc.gaps(F))
    x = np.cumsum(np.r_[np.zeros((1, 3)), rng.normal(size=(F - 1, 3)) * np.sqrt(0.3 ** 2 * dt)[:, None]], axis=0)
    cnt = np.full(F, m)
    cnt[[5, 6, 20]] = 0                             # frames without measurements
    ybar = np.stack([x[f] + rng.normal(size=(max(c, 1), 3)).mean(axis=0) * 0.8 if c else np.zeros(3) for f, c in enumerate(cnt)])
    # (the scatter of a frame's measurements about their mean is a constant of the data: part of data_cost at every x)
    scatter = float(sum(rng.chisquare(3 * (c - 1)) * 0.8 ** 2 for c in cnt if c > 1))
    return dt, cnt, ybar, scatter


def _toy_pieces(dt, cnt, ybar, scatter, q, s_t):
    """H (unscaled, data variance 1) at the effective variance s_t / q, the estimate, data cost and the exact log marginal likelihood"""
    F = len(cnt)
    et2 = s_t / q
    D = np.zeros((F, F))
    for f in range(F - 1):
        w = 1.0 / (et2 * dt[f])
        D[f, f] += w; D[f + 1, f + 1] += w; D[f, f + 1] -= w; D[f + 1, f] -= w
    H1 = np.diag(cnt.astype(np.float64)) + D        # per axis; the three axes are independent copies
    xh = np.linalg.solve(H1, cnt[:, None] * ybar)
    data = float(np.sum(cnt[:, None] * (ybar - xh) ** 2)) + scatter
    d = np.diff(xh, axis=0)
    prior = float(np.sum(d * d / (et2 * dt)[:, None]))
    n_y = 3 * int(cnt.sum())
    _, logdet = np.linalg.slogdet(H1 / q)
    loglik = (-0.5 * n_y * np.log(2 * np.pi * q) - 1.5 * (F - 1) * np.log(2 * np.pi * s_t) - 1.5 * np.sum(np.log(dt)) - 0.5 * (data + prior) / q
              + 1.5 * F * np.log(2 * np.pi) - 1.5 * logdet)
    return H1, xh, data, float(loglik), n_y


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_no_m_step_decreases_the_exact_marginal_likelihood(seed):
    dt, cnt, ybar, scatter = _toy(seed)
    F = len(cnt)
    q, s_t = 1.0, 0.05 ** 2
    last = None
    for it in range(25):
        H1, xh, data, loglik, n_y = _toy_pieces(dt, cnt, ybar, scatter, q, s_t)
        if last is not None:
            assert loglik >= last - 1e-9 * abs(last), (it, loglik, last)
        last = loglik
        S = np.linalg.inv(H1)
        d = np.diff(xh, axis=0)
        A_t = float(np.sum(d * d / dt[:, None]))
        U_t = 3.0 * float(np.sum((np.diag(S)[:-1] + np.diag(S)[1:] - 2 * np.diag(S, 1)) / dt))
        U_d = 3.0 * F - U_t / (s_t / q)              # tr(H H^-1) = 3 F here: three unknowns per frame
        assert abs(U_d - 3.0 * float(np.sum(cnt * np.diag(S)))) <= 1e-9 * U_d
        q, _, s_t = fr.mstep([0.0, 0.0, A_t, U_t], data, U_d, q, 1.0, s_t, F, n_y / 8.0, estimate=(1, 0, 1))
    print("seed %d: sigma_px %.4f (0.8), sigma_trans %.4f (0.3), log likelihood %.6f" % (seed, np.sqrt(q), np.sqrt(s_t), last))


# ---- 3. recovery ----
@pytest.mark.parametrize("seed", fc.WALK_SEEDS)
def test_recovery_of_a_simulated_random_walk(seed):
    ds, x0 = fc.walk(seed)
    td = tr.TrackData(ds, x0)
    r = fr.fit(fr.FitProblem(td), td.z0, SROT, STRANS)
    dev = np.array([r["sigma_px"], r["sigma_rot"], r["sigma_trans"]]) / fc.WALK_SIGMAS - 1.0
    print("seed %d: %d EM iterations (exit %d), deviations %s, caps %s" % (seed, r["iterations"], r["stop_code"], np.array2string(dev, precision=5),
                                                                          np.array2string(np.array(fc.CAPS), precision=5)))
    assert r["stop_code"] == 1
    assert np.all(np.abs(dev) <= fc.CAPS), (dev, fc.CAPS)


# ---- 4. aar_smooth_fit_params on the host ----
def test_default_fit_params():
    p = aar.smooth_fit_params()
    assert p.struct_size == C.sizeof(aar.CSmoothFitParams) == 32
    assert (p.max_iters, p.rel_tol, p.estimate_px, p.estimate_rot, p.estimate_trans) == (50, 1e-3, 1, 1, 1)
    aar.smooth_fit_params_validate()
    aar.smooth_fit_params_validate(rel_tol=0.0, max_iters=1, estimate_px=0, estimate_rot=0)


@pytest.mark.parametrize("bad, word", [(dict(max_iters=0), "max_iters"), (dict(max_iters=-3), "max_iters"), (dict(rel_tol=-1e-3), "rel_tol"),
                                       (dict(rel_tol=float("nan")), "rel_tol"), (dict(rel_tol=float("inf")), "rel_tol"),
                                       (dict(estimate_px=2), "estimate_px"), (dict(estimate_rot=-1), "estimate_rot"),
                                       (dict(estimate_trans=7), "estimate_trans"),
                                       (dict(estimate_px=0, estimate_rot=0, estimate_trans=0), "estimate_px, estimate_rot and estimate_trans")])
def test_invalid_fit_params_name_the_field(bad, word):
    with pytest.raises(aar.AarError) as e:
        aar.smooth_fit_params_validate(**bad)
    assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), str(e.value)


def test_fit_params_are_size_versioned():
    # a caller compiled against a shorter struct: the fields beyond its struct_size are at their defaults, whatever the memory holds
    cut = aar.CSmoothFitParams.estimate_px.offset
    aar.smooth_fit_params_validate(struct_size=cut, estimate_px=0, estimate_rot=0, estimate_trans=0)
    aar.smooth_fit_params_validate(struct_size=aar.CSmoothFitParams.rel_tol.offset, rel_tol=-1.0)
    aar.smooth_fit_params_validate(struct_size=4, max_iters=0)
    with pytest.raises(aar.AarError) as e:
        aar.smooth_fit_params_validate(struct_size=cut, max_iters=0)           # ... and those within it are read
    assert "max_iters" in str(e.value)
    with pytest.raises(aar.AarError) as e:
        aar.smooth_fit_params_validate(struct_size=2)
    assert e.value.code == aar.AAR_ERR_INVALID and "struct_size" in str(e.value)
    with pytest.raises(aar.AarError) as e:
        aar._check(aar.lib().aar_smooth_fit_params_validate(None))
    assert "null" in str(e.value)
