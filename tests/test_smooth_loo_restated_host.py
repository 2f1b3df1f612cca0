"""The float64 restatement of the smoothed track's per-detection layer (tests/smooth_loo_restated.py) held to routes that
never form (I - C_i)^-1, and its planted faults.  CPU only, numpy only.

  (a) the linear problem: LooSystem over the frame poses with the motion prior as H_p reproduces the smoother's H and the layer's C_i
  (b) the identities: Woodbury, q_i = the drop of the minimal cost, I + C_(i) = (I - C_i)^-1, Cook's distance by the moved solution, F
  (c) sum_i tr(C_i) = 6 F - tr(Sigma H_p)
  (d) every planted fault breaks a bar the clean layer passes
  (e) the planted outlier: first by F, not first by raw error -- random walk: rank 0 by F, rank 6 by e_d; constant velocity: 0 and 1
  (f) the second-order gap of q_i against a deletion and a re-smooth: smooth_loo_restated.GAP_Q
"""
import numpy as np
import pytest

import aar
import loo_restated as lr
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_loo_restated as sl

IDENTITY_BAR = 1e-9          # relative: dense 6F x 6F solves in float64 at kappa ~ 1e5
MODELS = {"rw": dict(model="rw"), "cv": dict(model="cv", sigma_rot0=cc.SROT0, sigma_trans0=cc.STRANS0)}


def _case(model, F=4, delta=None):
    ds = aar.synth(2, num_frames=F)
    x = sc.track_start(ds)
    sp = sl.problem(ds, x, cc.SROT, cc.STRANS, frame_time=cc.gaps(F), delta=delta, **MODELS[model])
    H, cost = sl.dense_system(sp, sl.frames_of(ds, x))
    return ds, x, sl.SmoothLoo(ds, x, H, cost, huber_delta=delta)


@pytest.fixture(scope="module", params=["rw", "cv"])
def case(request):
    ds, x, S = _case(request.param)
    return request.param, ds, x, S, S.loo_system(), S.all_C()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_the_linear_problem_is_the_smoothers(case):
    _, ds, x, S, ls, (C, s) = case
    assert _rel(ls.H, S.H) <= 1e-12                      # data blocks from the complex-step G plus H_p: the restated H again
    assert np.linalg.eigvalsh(S.H)[0] > 0
    for i in (0, S.N // 2, S.N - 1):
        assert _rel(ls.C(i), C[i]) <= IDENTITY_BAR
    assert S.nu == 8 * S.N - 6


def test_identities_without_the_inverse(case):
    _, ds, x, S, ls, (C, s) = case
    lev = np.trace(C, axis1=1, axis2=2)
    for i in sorted({int(np.argmax(lev)), int(np.argmin(lev)), S.N // 3}):
        Cd, w_d, drop, cost_d, k_d = ls.deleted(i)
        w, q, k, margin, und = lr.tail(C[i], ls.rho[i])
        assert not und and 0 < margin <= 1
        assert _rel(w, w_d) <= IDENTITY_BAR                                          # Woodbury
        assert abs(q - drop) <= IDENTITY_BAR * ls.cost_min                           # the drop of the minimal cost
        assert _rel(np.eye(8) + Cd, np.linalg.inv(np.eye(8) - C[i])) <= IDENTITY_BAR  # the gate of the reduced system
        assert abs(k - k_d) <= IDENTITY_BAR * max(abs(k_d), 1.0)                     # Cook's distance by the moved solution
        F, cook = lr.statistics(np.array([q]), np.array([k]), ls.cost_min, S.nu, 6 * S.F)
        assert abs(F[0] - (q / 8) / (cost_d / (S.nu - 8))) <= IDENTITY_BAR * F[0]
        assert abs(cook[0] - k_d / (6 * S.F * ls.cost_min / S.nu)) <= IDENTITY_BAR * cook[0]


def test_leverage_identity(case):
    _, ds, x, S, ls, (C, s) = case
    got, want = S.leverage_identity(C)
    assert abs(got - want) <= IDENTITY_BAR * 6 * S.F
    assert 0 < got < 6 * S.F                                                         # the prior determines part of every pose


@pytest.mark.parametrize("fault", sl.FAULTS)
def test_planted_faults_break_the_bars(fault):
    ds, x, S = _case("rw", delta=0.8 if fault == "huber_g" else None)
    C, s = S.all_C()
    bar = sl.certificate_bar(s)
    if fault in ("no_prior", "lag_block", "huber_g"):
        Cf, _ = S.all_C(fault)
        assert (np.abs(Cf - C) > bar[:, None, None]).any(axis=(1, 2)).sum() >= (1 if fault == "huber_g" else S.N // 2)
        return
    ls = S.loo_system()
    i = int(np.argmax(np.trace(C, axis1=1, axis2=2)))
    Cd, w_d, drop, cost_d, k_d = ls.deleted(i)
    w, q, k, _, _ = lr.tail(C[i], ls.rho[i])
    wf, qf, kf, _, _ = lr.tail(C[i], ls.rho[i], 3, fault)
    F, _ = lr.statistics(np.array([q]), np.array([k]), ls.cost_min, S.nu, 6 * S.F)
    Ff, _ = lr.statistics(np.array([qf]), np.array([kf]), ls.cost_min, S.nu, 6 * S.F, fault)
    want = (drop / 8) / (cost_d / (S.nu - 8))
    assert abs(F[0] - want) <= IDENTITY_BAR * want and _rel(w, w_d) <= lr.solve_bar(C[i])
    if fault == "c_sign":
        assert _rel(wf, w_d) > lr.solve_bar(C[i])
    assert abs(Ff[0] - want) > IDENTITY_BAR * want


@pytest.fixture(scope="module", params=["rw", "cv"])
def planted(request):
    P = sl.PLANT
    ds, x0, i = sl.planted()
    kw = sl.PLANT_MODELS[request.param]
    sp = sl.problem(ds, x0, P["sigma_rot"], P["sigma_trans"], **kw)
    run = sl.converged(sp, sl.frames_of(ds, x0), **sl.PLANT_LM)
    x = sl.with_frames(ds, x0, run["z"])
    H, cost = sl.dense_system(sp, run["z"])
    return request.param, ds, x, i, run, sl.SmoothLoo(ds, x, H, cost)


def test_planted_outlier_is_first_by_F_and_not_by_raw_error(planted):
    model, ds, x, i, run, S = planted
    Q = S.quantities(f_max=sl.PLANT_F_MAX)
    rank_f, rank_e = sl.ranks(Q["F"], i), sl.ranks(S.det_err(), i)
    print("%s: planted detection %d: rank by F %d (F = %.4f), rank by raw error %d (e_d = %.4f px, largest %.4f px)" %
          (model, i, rank_f, Q["F"][i], rank_e, S.det_err()[i], S.det_err().max()))
    assert rank_f == 0 and rank_e == {"rw": 6, "cv": 1}[model]
    assert Q["keep"][i] == 0 and Q["status"][i] == 0
    # the thin frame's other detection contradicts nothing but the shifted one: it is the only other rejection
    other = int(np.nonzero(np.asarray(ds.obs_frame) == sl.PLANT["frame"])[0][1])
    assert sorted(np.nonzero(Q["keep"] == 0)[0]) == sorted([i, other])


def test_second_order_gap_of_q(planted):
    model, ds, x, i, run, S = planted
    P = sl.PLANT
    Q = S.quantities()
    worst = 0.0
    for d in lr.three_detections(Q["leverage"], Q["q"]):
        dd = sl.without_detection(ds, d)
        sp = sl.problem(dd, x, P["sigma_rot"], P["sigma_trans"], **sl.PLANT_MODELS[model])
        rerun = sl.converged(sp, run["z"], **sl.PLANT_LM)
        gap = abs((S.cost - rerun["err"]) - Q["q"][d]) / Q["q"][d]
        print("%s: detection %d: q %.6f, drop %.6f, gap %.3e" % (model, d, Q["q"][d], S.cost - rerun["err"], gap))
        worst = max(worst, gap)
    assert worst <= sl.GAP_Q and worst >= 0.9 * sl.GAP_Q          # the constant is the measured value, not a loose cap


def test_undetermined_lone_detection():
    """one frame, one detection: V_0^-1 is the whole covariance, C a projector of rank 6: leverage 6, margin ~ 0, UNDETERMINED"""
    ds = aar.synth(2, num_frames=1)
    keep = np.zeros(ds.num_obs, dtype=np.uint8)
    keep[0] = 1
    ds = ds.select_observations(keep)
    x = sc.track_start(ds)
    for model in ("rw", "cv"):
        sp = sl.problem(ds, x, cc.SROT, cc.STRANS, **MODELS[model])
        H, cost = sl.dense_system(sp, sl.frames_of(ds, x))
        S = sl.SmoothLoo(ds, x, H, cost)
        Q = S.quantities(f_max=1.0)
        assert Q["status"][0] == lr.UNDETERMINED and Q["keep"][0] == 1 and abs(Q["leverage"][0] - 6) < 1e-6 and abs(Q["margin"][0]) < 1e-6
        assert np.isnan(Q["F"][0]) and np.isnan(Q["q"][0])


def test_smooth_loo_yaml_round_trip(tmp_path):
    """aar_smooth_loo_write_yaml (host code) in the dialect tests/test_loo_layers_host.py parses"""
    from conftest import load_golden
    from test_loo_layers_host import parse_loo_yaml
    ds, _ = load_golden("g2_small")
    N = ds.num_obs
    rng = np.random.default_rng(7)
    F = rng.uniform(0.0, 3.0, N)
    F[5], F[11] = 9.5, np.inf
    st = np.zeros(N, dtype=np.uint8)
    st[2] = aar.PREDICT_UNDETERMINED
    F[2] = np.nan
    keep = np.where((st == 0) & (F > 4.0), 0, 1).astype(np.uint8)
    rep = dict(num_residuals=8 * N + 6 * (ds.num_frames - 1), num_vars=6 * ds.num_frames, data_cost=12.5, prior_cost=0.75, sigma2=0.25, dof=8 * N - 6,
               behind=0, undetermined=1, rejected=int((keep == 0).sum()), f_max=4.0, max_f=np.inf, argmax_f=11, leverage_sum=93.5, launches=4, seconds=0.001, kernel_seconds=0.0)
    loo = aar.DetectionLoo(F=F, q=2 * F, leverage=rng.uniform(0.1, 4.0, N), status=st, keep=keep, report=rep)
    err = np.linspace(0.1, 2.0, N)
    path = str(tmp_path / "smooth_loo.yaml")
    aar.smooth_loo_write_yaml(path, ds, loo, err)
    y = parse_loo_yaml(path)
    assert (y["sigma2"], y["data_cost"], y["prior_cost"], y["dof"], y["f_max"], y["undetermined"], y["rejected"], y["leverage_sum"]) == \
        (0.25, 12.5, 0.75, 8 * N - 6, 4.0, 1, rep["rejected"], 93.5)
    assert np.isinf(y["max_f"])
    want = np.nonzero((keep == 0) | (st != 0))[0]
    assert [r[:3] for r in y["listed"]] == [(int(ds.frame_ids[ds.obs_frame[o]]), int(ds.cam_ids[ds.obs_cam[o]]), int(ds.marker_ids[ds.obs_marker[o]])) for o in want]
    np.testing.assert_allclose([r[5] for r in y["listed"]], loo.leverage[want], rtol=1e-6)
    np.testing.assert_allclose([r[6] for r in y["listed"]], err[want], rtol=1e-6)
    assert sum(v[0] for v in y["cameras"].values()) == N == sum(v[0] for v in y["markers"].values())
