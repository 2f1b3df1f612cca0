"""The per-detection layer of a smoothed track on the device (aar_track_smooth_detection_leverage, _detection_loo, _predict_corners,
_gate_detections; csrc/smooth_predict_kernels.hip).  Needs a real MI355X.  Both motion models on every shape.

A case is run ONCE per model (_run): the device's dense H and costs (aar_track_smooth_system2 at mu = 0), aar_track_smooth_covariance2,
aar_track_smooth_query2 at the frame times, the four new entries (predict_corners at the detections' own triples), the old entries again.

1. Certificate: C of predict_corners against tests/smooth_loo_restated.py fed the DEVICE's own query cov and the complex-step G:
   |C_dev - C_ref| <= (12 2^-53 + 2 SCALED_BAR) s, s = | |G| |Sigma| |G^T| |_F.  uv within ROW_BAR.  The tail's outputs within
   loo_restated.solve_bar (64 eps kappa_2(A)) of loo_restated.tail on the device's own C, in test_gpu_detection_loo's norms.
2. End to end: C against G inv(H) G^T with numpy.linalg.inv of the dense H: within FLAT_BAR = 1e-7 of s.
3. Bits: the diagonal of predict_corners at the detections' triples = row_leverage (constant velocity: after checking that query2's cov
   at a frame time is covariance2's block); leverage of the two entries; C symmetric; two calls; the old entries before and after.
4. The leverage identity sum tr(C_i) = 6 F - tr(Sigma H_prior), H_prior from the restatement.
5. Time queries on a frame time, inside a gap, before and after the recording; duplicates and a permutation; cov = NULL; the gate.
6. A camera turned away: bit 0, the neighbours in the same wavefront bit for bit as in a launch without it.
7. The planted outlier of tests/test_smooth_loo_restated_host.py (e) on the device's own smoothed track; q_i against a deletion and a
   re-smooth of three detections, 4 x smooth_loo_restated.GAP_Q.
8. Refusals leave 0x55-filled outputs and reports untouched.
"""
import ctypes as C

import numpy as np
import pytest

import aar
import loo_restated as lr
import predict_restated as prs
import smooth_cases as sc
import smooth_cv_restated as cv
import smooth_loo_restated as sl
import smooth_relative_cases as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = lr.U53
SROT, STRANS = rc.SROT, rc.STRANS
ROW_BAR = 1e-9             # the project's bar for double-mode rows, in pixels (tests/test_gpu_observation_passes.py)
MODELS = ["rw", "cv"]
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _first(ds, counts):
    """the first counts[f] detections of frame f (frames beyond the list: none)"""
    fr = np.asarray(ds.obs_frame)
    keep = np.zeros(ds.num_obs, dtype=np.uint8)
    for f, n in enumerate(counts):
        keep[np.nonzero(fr == f)[0][:n]] = 1
    out = ds.select_observations(keep)
    assert out.num_obs == sum(counts)
    return out


# N = 1, 7, 8, 9, 65: a lone group, a wavefront short by one, exactly one wavefront, a second wavefront with one live group, nine wavefronts;
# F = 1 .. 5 (4 and 5 with their end frames emptied), 33 with the emptied run of ten, 515 above the one-launch reduction
CASES = {
    "n1_f1": lambda: _first(aar.synth(2, num_frames=1), [1]),
    "n2_f1": lambda: _first(aar.synth(2, num_frames=1), [2]),
    "n7_f2": lambda: _first(aar.synth(2, num_frames=2), [4, 3]),
    "n8_f2": lambda: _first(aar.synth(2, num_frames=2), [4, 4]),
    "n9_f3": lambda: _first(aar.synth(2, num_frames=3), [3, 3, 3]),
    "n65_f17": lambda: _first(aar.synth(2, num_frames=17), [4, 4, 4, 4, 5, 5, 5, 5, 5, 5, 3, 3, 3, 3, 3, 3, 1]),
    "f2": lambda: rc.dataset(2), "f3": lambda: rc.dataset(3), "f4": lambda: rc.dataset(4), "f5": lambda: rc.dataset(5),
    "f33": lambda: rc.dataset(33),
    "big": rc.big_dataset,
}
NAMES = list(CASES)


class Run:
    pass


def _kw(model, F):
    return dict(frame_time=rc.times(F), **rc.MODELS[model])


def _run(name, model):
    key = (name, model)
    if key in _RUNS:
        return _RUNS[key]
    r = Run()
    r.ds = ds = CASES[name]()
    r.x = x = sc.track_start(ds)
    F = r.F = ds.num_frames
    r.kw = kw = _kw(model, F)
    r.ft = np.arange(F, dtype=np.float64) if kw["frame_time"] is None else np.asarray(kw["frame_time"], dtype=np.float64)
    r.q3 = prs.detection_queries(ds)
    qc, qm, qt = r.q3[:, 0], r.q3[:, 1], r.ft[r.q3[:, 2]]
    with aar.Problem(ds) as p:
        gd, go, go2, _, _, r.cost = p.track_smooth_system2(x, SROT, STRANS, 0.0, **kw)
        r.H = cv.dense(gd, go, go2)
        r.cov2 = p.track_smooth_covariance2(x, SROT, STRANS, lag2=model == "cv", **kw)
        r.qry = p.track_smooth_query2(x, SROT, STRANS, r.ft, **kw)
        r.lev, r.rows, r.lrep = p.track_smooth_detection_leverage(x, SROT, STRANS, rows=True, **kw)
        r.loo = p.track_smooth_detection_loo(x, SROT, STRANS, **kw)
        r.uv, r.cov, r.st, r.seg, r.prep = p.track_smooth_predict_corners(x, SROT, STRANS, qc, qm, qt, **{k: v for k, v in kw.items() if k != "rel_motion"})
        r.loo2 = p.track_smooth_detection_loo(x, SROT, STRANS, f_max=sl.PLANT_F_MAX, **kw)
        r.cov2_after = p.track_smooth_covariance2(x, SROT, STRANS, lag2=model == "cv", **kw)
        r.qry_after = p.track_smooth_query2(x, SROT, STRANS, r.ft, **kw)
    r.S = sl.SmoothLoo(ds, x, r.H, r.cost, frame_cov=r.qry[1])          # the restatement fed the device's own blocks
    r.Cref, r.s = r.S.all_C()
    _RUNS[key] = r
    return r


def _certify_tail(C, r, loo, sel, num_vars):
    """worst ratios (w, q, k) to the bars of tests/test_gpu_detection_loo.py's certificate over the detections sel"""
    rep = loo.report
    cook_den = num_vars * rep["sigma2"]
    out = np.zeros(3)
    for i in sel:
        A = np.eye(8) - C[i]
        w_ref = np.linalg.solve(A, r[i])
        q_ref, k_ref = float(r[i] @ w_ref), float(w_ref @ C[i] @ w_ref)
        nw, nr, nC = np.linalg.norm(w_ref), np.linalg.norm(r[i]), np.linalg.norm(C[i], 2)
        bw = lr.solve_bar(C[i])
        out = np.maximum(out, [np.linalg.norm(loo.loo_resid[i] - w_ref) / (bw * nw), abs(loo.q[i] - q_ref) / ((bw + 16 * EPS) * nr * nw),
                               abs(loo.cook[i] * cook_den - k_ref) / ((2 * bw + 80 * EPS) * nC * nw * nw)])
    return out


# ---- 1. certificate ----
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_certificate(model, name):
    r = _run(name, model)
    S, loo, N, F = r.S, r.loo, r.ds.num_obs, r.F
    assert (r.st == 0).all() and ((loo.status & 3) == 0).all() and r.cov.shape == (N, 8, 8)
    err = np.abs(r.cov - r.Cref).max(axis=(1, 2)) / sl.certificate_bar(r.s)
    duv = float(np.abs(r.uv.reshape(-1, 8) - S.uv).max())
    print("%s %s: N %d F %d: |C_dev - C_ref| / bar %.3e, uv %.3e px" % (name, model, N, F, err.max(), duv))
    assert err.max() <= 1.0 and duv <= ROW_BAR
    assert np.array_equal(r.cov, np.swapaxes(r.cov, 1, 2))
    # the tail on the device's own C and the device's own corners
    rr = S.obs - r.uv.reshape(-1, 8)
    sel = np.nonzero(loo.status == 0)[0]
    und = np.nonzero(loo.status == aar.PREDICT_UNDETERMINED)[0]
    assert len(sel) + len(und) == N
    if name == "n1_f1":
        assert list(und) == [0] and abs(loo.leverage[0] - 6) <= 1e-6 and abs(loo.margin[0]) <= 1e-6
    else:
        assert len(und) == 0
    if name == "big":
        sel = sel[:: max(len(sel) // 256, 1)]
    ratios = _certify_tail(r.cov, rr, loo, sel, 6 * F)
    print("%s %s: tail: worst ratio to the bar w %.3e q %.3e k %.3e; margin %.3g .. %.3g" %
          (name, model, ratios[0], ratios[1], ratios[2], np.nanmin(loo.margin), np.nanmax(loo.margin)))
    assert ratios.max() <= 1.0
    for i in list(sel[:32]) + list(und):
        _, _, _, mg, u = lr.tail(r.cov[i], rr[i])
        assert u == (loo.status[i] == aar.PREDICT_UNDETERMINED) and abs(loo.margin[i] - mg) <= 64 * EPS * max(1.0, np.linalg.norm(r.cov[i], 2))
    assert np.isnan(loo.loo_resid[und]).all() and np.isnan(loo.q[und]).all() and np.isnan(loo.F[und]).all() and np.isnan(loo.cook[und]).all()
    assert np.isfinite(loo.leverage).all() and np.isfinite(loo.margin).all() and (loo.keep == 1).all()
    # F and cook from q, k and the report's scalars
    rep = loo.report
    nu = 8 * N - 6
    assert rep["dof"] == nu and rep["num_vars"] == 6 * F and (rep["data_cost"], rep["prior_cost"]) == tuple(r.cost)
    cost = r.cost[0] + r.cost[1]
    Fr, ck = lr.statistics(loo.q, loo.cook * (6 * F * rep["sigma2"]), cost, nu, 6 * F)
    ok = np.isfinite(Fr)
    assert np.array_equal(np.isnan(Fr), np.isnan(loo.F)) and (np.abs(loo.F[ok] - Fr[ok]) <= 8 * EPS * np.abs(Fr[ok])).all()
    # the report and the rule
    assert rep["undetermined"] == len(und) and rep["rejected"] == 0 and rep["behind"] == 0 and np.isinf(rep["f_max"])
    Fm = np.where(np.isnan(loo.F), -np.inf, loo.F)
    if np.isfinite(Fm).any() or np.isposinf(Fm).any():
        assert rep["argmax_f"] == int(np.argmax(Fm)) and rep["max_f"] == loo.F[rep["argmax_f"]]
    else:
        assert rep["argmax_f"] == -1 and np.isnan(rep["max_f"])
    assert rep["leverage_sum"] == r.lrep["leverage_sum"] and rep["launches"] == r.lrep["launches"] == r.cov2[-1]["launches"] + 1
    l2 = r.loo2
    assert np.array_equal(l2.keep == 0, (l2.status == 0) & (l2.F > sl.PLANT_F_MAX)) and l2.report["rejected"] == int((l2.keep == 0).sum())
    for a, b in ((l2.loo_resid, loo.loo_resid), (l2.q, loo.q), (l2.F, loo.F), (l2.cook, loo.cook), (l2.leverage, loo.leverage), (l2.margin, loo.margin)):
        assert np.array_equal(a, b, equal_nan=True)
    if name == "big":
        assert aar.lib().aar_smooth_solve_launches(F, 1 if model == "cv" else 0) > 1


# ---- 2. end to end ----
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_end_to_end(model, name):
    r = _run(name, model)
    S = sl.SmoothLoo(r.ds, r.x, r.H, r.cost)          # Sigma = numpy.linalg.inv of the dense H
    Cref, s = S.all_C()
    ratio = np.abs(r.cov - Cref).max(axis=(1, 2)) / s
    print("%s %s: |C_dev - G inv(H) G^T| / s %.3e (kappa %.3e)" % (name, model, ratio.max(), np.linalg.cond(r.H)))
    assert ratio.max() <= sl.FLAT_BAR
    # 4. the leverage identity, H_prior from the restatement: every trace within sqrt(8) times its block's bar
    got, want = float(r.lev.sum()), S.leverage_identity(Cref)[1]
    assert abs(got - want) <= np.sqrt(8.0) * sl.FLAT_BAR * s.sum(), (got, want)
    assert r.lrep["leverage_sum"] == float(np.cumsum(r.lev)[-1])


# ---- 3. bits ----
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_bits(model, name):
    r = _run(name, model)
    # query2's cov at a frame time is covariance2's block: checked first, the rest stands on it
    assert np.array_equal(r.qry[1], r.cov2[0]) and np.array_equal(r.qry[0], sl.frames_of(r.ds, r.x))
    assert np.array_equal(np.diagonal(r.cov, axis1=1, axis2=2), r.rows)
    assert np.array_equal(r.lev, r.loo.leverage) and np.array_equal(r.lev, prs.trace_tree(r.cov))
    assert np.array_equal(r.seg, r.q3[:, 2]) and r.prep["num_on_frame"] == len(r.q3) and r.prep["num_inside"] == r.prep["num_outside"] == 0
    # the old entries before and after the new ones
    for a, b in zip(r.cov2[:-1], r.cov2_after[:-1]):
        assert (a is None and b is None) or np.array_equal(a, b)
    for a, b in zip(r.qry[:3], r.qry_after[:3]):
        assert np.array_equal(a, b)
    # two calls
    qc, qm, qt = r.q3[:, 0], r.q3[:, 1], r.ft[r.q3[:, 2]]
    with aar.Problem(r.ds) as p:
        lev, rows, _ = p.track_smooth_detection_leverage(r.x, SROT, STRANS, rows=True, **r.kw)
        loo = p.track_smooth_detection_loo(r.x, SROT, STRANS, **r.kw)
        uv, cov, st, _, _ = p.track_smooth_predict_corners(r.x, SROT, STRANS, qc, qm, qt, **r.kw)
        with pytest.raises(aar.AarError):
            p.lm_step()          # no LM state is left behind
    assert np.array_equal(lev, r.lev) and np.array_equal(rows, r.rows) and np.array_equal(uv, r.uv) and np.array_equal(cov, r.cov)
    for k in ("loo_resid", "q", "F", "cook", "leverage", "margin", "status", "keep"):
        assert np.array_equal(getattr(loo, k), getattr(r.loo, k), equal_nan=True), k


def test_bundle_loo_bits_before_and_after():
    ds, _ = load_golden("g2_small")
    x = np.asarray(ds.x_full, dtype=np.float64)
    with aar.Problem(ds, solver="direct", deterministic=True) as p:
        a = p.detection_loo(x)
        for model in MODELS:
            kw = _kw(model, ds.num_frames)
            p.track_smooth_detection_leverage(x, SROT, STRANS, **kw)
            p.track_smooth_detection_loo(x, SROT, STRANS, **kw)
            p.track_smooth_predict_corners(x, SROT, STRANS, [0], [0], [0.5], **kw)
            p.track_smooth_gate_detections(x, SROT, STRANS, [0], [0], [0.5], np.zeros((1, 8)), **kw)
        b = p.detection_loo(x)
    for k in ("loo_resid", "q", "F", "cook", "leverage", "margin", "status", "keep"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k


# ---- 5. time queries ----
def _time_queries(r, n, seed):
    """n (camera, marker, time): the frame times, the middles of gaps, before and after the recording, cycled"""
    rng = np.random.default_rng(seed)
    ft, F = r.ft, r.F
    pool = list(ft) + [0.5 * (ft[f] + ft[f + 1]) for f in range(F - 1)] + [ft[0] - 0.75, ft[-1] + 1.25, ft[0] + 0.3 * (ft[-1] - ft[0]) + 0.01]
    t = np.array([pool[i % len(pool)] for i in range(n)])
    return rng.integers(0, r.ds.num_cams, n), rng.integers(0, r.ds.num_markers, n), t


@pytest.mark.parametrize("name", ["n2_f1", "f2", "f5", "f33"])
@pytest.mark.parametrize("model", MODELS)
def test_time_queries(model, name):
    r = _run(name, model)
    n = 131
    qc, qm, qt = _time_queries(r, n, 5)
    rng = np.random.default_rng(9)
    with aar.Problem(r.ds) as p:
        pose, pcov, seg0, qrep = p.track_smooth_query2(r.x, SROT, STRANS, qt, **r.kw)
        uv, cov, st, seg, rep = p.track_smooth_predict_corners(r.x, SROT, STRANS, qc, qm, qt, **r.kw)
        uv1, none, st1, seg1, rep1 = p.track_smooth_predict_corners(r.x, SROT, STRANS, qc, qm, qt, covariance=False, **r.kw)
        obs = (uv.reshape(n, 8) + rng.normal(0, 0.7, (n, 8))).astype(np.float32)
        inn, m2, stg, segg, grep = p.track_smooth_gate_detections(r.x, SROT, STRANS, qc, qm, qt, obs, **r.kw)
        # duplicates and a permutation: the same bits per query
        perm = rng.permutation(n)
        idx = np.r_[perm, perm[:7], 3, 3]
        uvp, covp, stp, segp, _ = p.track_smooth_predict_corners(r.x, SROT, STRANS, qc[idx], qm[idx], qt[idx], **r.kw)
        innp, m2p, _, _, _ = p.track_smooth_gate_detections(r.x, SROT, STRANS, qc[idx], qm[idx], qt[idx], obs[idx], **r.kw)
    assert (st == 0).all() and np.array_equal(seg, seg0) and np.array_equal(seg1, seg0) and np.array_equal(segg, seg0)
    uvr, G, depth = sl.corners_at(r.ds, r.x, qc, qm, pose)
    assert (depth > 0).all()
    Cref, s = sl.push(G, pcov)
    err = np.abs(cov - Cref).max(axis=(1, 2)) / sl.certificate_bar(s)
    print("%s %s: %d time queries (%d inside, %d on a frame, %d outside): |C - C_ref| / bar %.3e, uv %.3e px" %
          (name, model, n, rep["num_inside"], rep["num_on_frame"], rep["num_outside"], err.max(), np.abs(uv.reshape(n, 8) - uvr).max()))
    assert err.max() <= 1.0 and np.abs(uv.reshape(n, 8) - uvr).max() <= ROW_BAR
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2)) and np.array_equal(uv1, uv) and none is None and np.array_equal(st1, st)
    assert (rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (qrep["num_inside"], qrep["num_on_frame"], qrep["num_outside"])
    assert rep["num_outside"] >= 2 and rep["num_on_frame"] >= r.F and (r.F == 1 or rep["num_inside"] >= r.F - 1)
    assert rep["launches"] == qrep["launches"] + 1 and (rep["data_cost"], rep["prior_cost"]) == tuple(r.cost)
    assert rep1["launches"] == (3 if model == "rw" else rep["launches"])          # random walk without cov: one unpack, the queries, the corners: no chain
    assert rep["leverage_sum"] == float(np.cumsum(prs.trace_tree(cov))[-1])
    # the gate on the device's own C and corners
    e = obs.astype(np.float64) - uv.reshape(n, 8)
    assert np.array_equal(inn, e) and (stg == 0).all() and grep["leverage_sum"] == 0
    for i in range(n):
        A = np.eye(8) + cov[i]
        w = np.linalg.solve(A, e[i])
        assert abs(m2[i] - e[i] @ w) <= (lr.solve_bar(cov[i], 4) + 16 * EPS) * np.linalg.norm(e[i]) * np.linalg.norm(w)
    assert np.array_equal(uvp, uv[idx]) and np.array_equal(covp, cov[idx]) and np.array_equal(segp, seg[idx])
    assert np.array_equal(innp, inn[idx]) and np.array_equal(m2p, m2[idx])


# ---- 6. a camera turned away ----
@pytest.mark.parametrize("model", MODELS)
def test_camera_turned_away(model):
    ds0 = rc.dataset(5)
    c = [k for k in range(ds0.num_cams) if k != ds0.root_cam][0]
    keep = (np.asarray(ds0.obs_cam) != c).astype(np.uint8)
    ds = ds0.select_observations(keep)          # the camera sees nothing, so H does not depend on where it looks
    x = sc.track_start(ds)
    o = 6 * (c - (c > ds.root_cam))
    x[o:o + 3] = aar.rodrigues_mat2vec(aar.rodrigues_vec2mat(x[o:o + 3]) @ np.diag([-1.0, 1.0, -1.0]))          # half a turn about its own y axis
    xt = x.copy()
    kw = _kw(model, ds.num_frames)
    n = 24
    rng = np.random.default_rng(4)
    qc, qm = rng.integers(0, ds.num_cams, n), rng.integers(0, ds.num_markers, n)
    qc[[2, 9, 10, 17]] = c          # inside wavefronts 0, 1 and 2, two of them neighbours
    away = qc == c
    qt = rng.uniform(-1.0, rc.times(5)[-1] + 1.0, n)
    obs = rng.normal(500, 100, (n, 8)).astype(np.float32)
    with aar.Problem(ds) as p:
        uv, cov, st, seg, rep = p.track_smooth_predict_corners(xt, SROT, STRANS, qc, qm, qt, **kw)
        inn, m2, stg, _, _ = p.track_smooth_gate_detections(xt, SROT, STRANS, qc, qm, qt, obs, **kw)
        # the launch without them: the same wavefront slots, the turned camera's queries replaced by another camera's
        qc2 = np.where(away, ds.root_cam, qc)
        uv2, cov2, st2, _, _ = p.track_smooth_predict_corners(xt, SROT, STRANS, qc2, qm, qt, **kw)
        inn2, m22, _, _, _ = p.track_smooth_gate_detections(xt, SROT, STRANS, qc2, qm, qt, obs, **kw)
        # ... and packed: other neighbours, other wavefronts
        uv3, cov3, st3, _, _ = p.track_smooth_predict_corners(xt, SROT, STRANS, qc[~away], qm[~away], qt[~away], **kw)
    assert np.array_equal(st, away.astype(np.uint8)) and np.array_equal(stg, st) and rep["behind"] == int(away.sum()) and (st2 == 0).all()
    assert np.isnan(uv[away]).all() and np.isnan(cov[away]).all() and np.isnan(inn[away]).all() and np.isnan(m2[away]).all()
    assert np.isfinite(uv[~away]).all() and np.isfinite(cov[~away]).all() and np.isfinite(m2[~away]).all()
    assert np.array_equal(uv[~away], uv2[~away]) and np.array_equal(cov[~away], cov2[~away])
    assert np.array_equal(inn[~away], inn2[~away]) and np.array_equal(m2[~away], m22[~away])
    assert np.array_equal(uv[~away], uv3) and np.array_equal(cov[~away], cov3) and (st3 == 0).all()


# ---- 7. the planted outlier, and q against a deletion and a re-smooth ----
@pytest.mark.parametrize("model", MODELS)
def test_planted_outlier_and_deletion(model):
    P = sl.PLANT
    ds, x0, i = sl.planted()
    kw = sl.PLANT_MODELS[model]
    lm = aar.lm_default_params()
    lm.min_average_step_error_diff = 0.0
    lm.max_iters = 30
    with aar.Problem(ds) as p:
        x, srep, _, _ = p.track_smooth(x0, P["sigma_rot"], P["sigma_trans"], params=lm, **kw)
        loo = p.track_smooth_detection_loo(x, P["sigma_rot"], P["sigma_trans"], f_max=sl.PLANT_F_MAX, **kw)
        err = p.residual_report(x).det_err
    rank_f, rank_e = sl.ranks(loo.F, i), sl.ranks(err, i)
    other = int(np.nonzero(np.asarray(ds.obs_frame) == P["frame"])[0][1])
    print("%s: planted detection %d: rank by F %d (F = %.4f, next %.4f), rank by raw error %d of %d (e_d = %.4f px)" %
          (model, i, rank_f, loo.F[i], np.sort(loo.F)[-2], rank_e, ds.num_obs, err[i]))
    assert rank_f == 0 and rank_e == {"rw": 6, "cv": 1}[model]
    assert sorted(np.nonzero(loo.keep == 0)[0]) == sorted([i, other]) and (loo.status == 0).all()
    rep = loo.report
    assert rep["rejected"] == 2 and rep["undetermined"] == 0 and rep["argmax_f"] == i and rep["max_f"] == loo.F[i] and rep["f_max"] == sl.PLANT_F_MAX
    cost = rep["data_cost"] + rep["prior_cost"]
    worst = 0.0
    for d in lr.three_detections(loo.leverage, loo.q):
        with aar.Problem(sl.without_detection(ds, d)) as p:
            _, rr, _, _ = p.track_smooth(x, P["sigma_rot"], P["sigma_trans"], params=lm, **kw)
        drop = cost - rr["final_cost"]
        gap = abs(drop - loo.q[d]) / loo.q[d]
        print("%s: detection %d: q %.6f, drop %.6f, gap %.3e (reference %.3e)" % (model, d, loo.q[d], drop, gap, sl.GAP_Q))
        worst = max(worst, gap)
    assert worst <= 4 * sl.GAP_Q


# ---- 8. refusals ----
def _raw(p, entry, x, sp, n, rule=None, qc=None, qm=None, qt=None, obs=None, rep_size=None):
    """(code, every output and the report still 0x55-filled) of one raw call"""
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    m = max(n, 1)
    d8, d64, d1 = [np.frombuffer(b"\x55" * (8 * k * m), dtype=np.float64).copy() for k in (8, 64, 1)]
    ds_ = [np.frombuffer(b"\x55" * (8 * m), dtype=np.float64).copy() for _ in range(5)]
    u1, u2 = [np.frombuffer(b"\x55" * m, dtype=np.uint8).copy() for _ in range(2)]
    seg = np.frombuffer(b"\x55" * (4 * m), dtype=np.int32).copy()
    rep = (aar.CSmoothLooReport if entry == "loo" else aar.CSmoothPredictReport)()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep) if rep_size is None else rep_size
    P = lambda a: a.ctypes.data_as(dp)
    L = aar.lib()
    xs = P(x)
    if entry == "leverage":
        code = L.aar_track_smooth_detection_leverage(p.handle, xs, sp, P(d1), P(d8), C.byref(rep))
    elif entry == "loo":
        code = L.aar_track_smooth_detection_loo(p.handle, xs, sp, rule, P(d8), P(ds_[0]), P(ds_[1]), P(ds_[2]), P(ds_[3]), P(ds_[4]),
                                                u1.ctypes.data_as(up), u2.ctypes.data_as(up), C.byref(rep))
    elif entry == "predict":
        code = L.aar_track_smooth_predict_corners(p.handle, xs, sp, n, qc.ctypes.data_as(ip), qm.ctypes.data_as(ip), P(qt), P(d8), P(d64),
                                                  u1.ctypes.data_as(up), seg.ctypes.data_as(ip), C.byref(rep))
    else:
        code = L.aar_track_smooth_gate_detections(p.handle, xs, sp, n, qc.ctypes.data_as(ip), qm.ctypes.data_as(ip), P(qt),
                                                  obs.ctypes.data_as(C.POINTER(C.c_float)) if obs is not None else None, P(d8), P(d1),
                                                  u1.ctypes.data_as(up), seg.ctypes.data_as(ip), C.byref(rep))
    body = bytes(bytearray(rep))[4:]
    untouched = all(bytes(a.tobytes()) == b"\x55" * a.nbytes for a in [d8, d64, d1, u1, u2, seg] + ds_) and body == b"\x55" * len(body)
    return code, untouched


def _all_entries(p, x, sp, ds, rule=None, qt=None):
    n = 5
    qc, qm = np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32)
    qt = np.linspace(0.0, 1.0, n) if qt is None else qt
    obs = np.zeros((n, 8), dtype=np.float32)
    return [_raw(p, "leverage", x, sp, ds.num_obs), _raw(p, "loo", x, sp, ds.num_obs, rule),
            _raw(p, "predict", x, sp, n, qc=qc, qm=qm, qt=qt), _raw(p, "gate", x, sp, n, qc=qc, qm=qm, qt=qt, obs=obs)]


@pytest.mark.parametrize("model", MODELS)
def test_refusals_leave_the_outputs_untouched(model):
    ds = rc.dataset(5)
    x = sc.track_start(ds)
    F = ds.num_frames
    mk = rc.MODELS[model]
    sp = aar.SmoothParams(SROT, STRANS, rc.times(F), None, None, mk["model"], mk.get("sigma_rot0", 0.0), mk.get("sigma_trans0", 0.0))
    msg = lambda: aar.lib().aar_last_error().decode()
    # a communicator: the smoother's own refusal
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm, solver="direct") as p:
            for code, untouched in _all_entries(p, x, C.byref(sp.c), ds):
                assert code == aar.AAR_ERR_UNSUPPORTED and untouched and "single-GPU only" in msg()
    finally:
        comm.close()
        group.close()
    with aar.Problem(ds, with_huber=True) as p:
        got = _all_entries(p, x, C.byref(sp.c), ds)
        assert got[1][0] == aar.AAR_ERR_UNSUPPORTED and got[1][1] and "with_huber" in msg() and "Gaussian" in msg()
        assert [g[0] for g in (got[0], got[2], got[3])] == [aar.AAR_OK] * 3          # the others ask nothing of the data model
    with aar.Problem(ds) as p:
        for bad in (0.0, -1.0, np.inf, np.nan):
            rule = aar.CLooRule()
            rule.struct_size, rule.f_max = C.sizeof(aar.CLooRule), bad
            code, untouched = _raw(p, "loo", x, C.byref(sp.c), ds.num_obs, C.byref(rule))
            assert code == aar.AAR_ERR_INVALID and untouched and "f_max" in msg(), bad
        n = 5
        qc, qm, qt = np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.linspace(0.0, 1.0, n)
        obs = np.zeros((n, 8), dtype=np.float32)
        bm = qm.copy()
        bm[2] = ds.num_markers
        bc = qc.copy()
        bc[4] = -1
        bt = qt.copy()
        bt[3] = np.inf
        for entry in ("predict", "gate"):
            code, untouched = _raw(p, entry, x, C.byref(sp.c), n, qc=qc, qm=bm, qt=qt, obs=obs)
            assert code == aar.AAR_ERR_INVALID and untouched and "q_marker[2]" in msg()
            code, untouched = _raw(p, entry, x, C.byref(sp.c), n, qc=bc, qm=qm, qt=qt, obs=obs)
            assert code == aar.AAR_ERR_INVALID and untouched and "q_cam[4]" in msg()
            code, untouched = _raw(p, entry, x, C.byref(sp.c), n, qc=qc, qm=qm, qt=bt, obs=obs)
            assert code == aar.AAR_ERR_INVALID and untouched and "query_time[3]" in msg()
        code, untouched = _raw(p, "gate", x, C.byref(sp.c), n, qc=qc, qm=qm, qt=qt, obs=None)
        assert code == aar.AAR_ERR_INVALID and untouched
        # a report whose struct_size is not set
        for code, untouched in [_raw(p, "leverage", x, C.byref(sp.c), ds.num_obs, rep_size=2), _raw(p, "loo", x, C.byref(sp.c), ds.num_obs, rep_size=2)]:
            assert code == aar.AAR_ERR_INVALID and untouched
        if model == "rw":          # (constant velocity refuses rel_motion as invalid parameters already)
            spr = aar.SmoothParams(SROT, STRANS, rc.times(F), np.zeros((F - 1, 6)), None, "rw")
            for entry in ("predict", "gate"):
                code, untouched = _raw(p, entry, x, C.byref(spr.c), n, qc=qc, qm=qm, qt=qt, obs=obs)
                assert code == aar.AAR_ERR_UNSUPPORTED and untouched and "rel_motion" in msg() and "no closed form" in msg()
    # a pivot of the chain: no detection in any frame, the prior alone is singular -- the chain's own message
    empty = sc.without_frames(ds, range(F))
    with aar.Problem(empty) as p:
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_covariance2(x, SROT, STRANS, lag2=False, frame_time=rc.times(F), **mk)
        assert e.value.code == aar.AAR_ERR_NUMERIC
        for code, untouched in _all_entries(p, x, C.byref(sp.c), empty):
            assert code == aar.AAR_ERR_NUMERIC and untouched and "non-positive pivot" in msg() and "elimination" in msg()
    # ... and the problem works on afterwards; every output may be NULL
    with aar.Problem(ds) as p:
        xs = x.ctypes.data_as(C.POINTER(C.c_double))
        assert aar.lib().aar_track_smooth_detection_loo(p.handle, xs, C.byref(sp.c), None, None, None, None, None, None, None, None, None, None) == aar.AAR_OK
        assert aar.lib().aar_track_smooth_predict_corners(p.handle, xs, C.byref(sp.c), 0, None, None, None, None, None, None, None, None) == aar.AAR_OK
        loo = p.track_smooth_detection_loo(x, SROT, STRANS, frame_time=rc.times(F), **mk)
        assert np.isfinite(loo.leverage).all()


# ---- 9. the other layers ----
@pytest.mark.parametrize("model", MODELS)
def test_mapper_by_id(tmp_path, model):
    import os
    import subprocess
    from conftest import PKG, ROOT
    exe = str(tmp_path / "smooth_loo_mapper_main")
    cc_ = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_loo_mapper_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                          "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr
    ds = aar.synth(2)
    kw = rc.MODELS[model]
    ft = np.asarray(ds.frame_ids, dtype=np.float64)
    qc, qm, qt = [0, 2, 3, 1], [1, 5, 0, 7], [ft[3], 0.5 * (ft[10] + ft[11]), ft[0] - 2.0, ft[-1] + 0.25]
    ids = [str(v) for c, m, t in zip(qc, qm, qt) for v in (int(ds.cam_ids[c]), int(ds.marker_ids[m]), repr(float(t)))]
    run = subprocess.run([exe, "2", model, repr(SROT), repr(STRANS), repr(kw.get("sigma_rot0", 0.0)), repr(kw.get("sigma_trans0", 0.0)), "2.5"] + ids,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = dict(ln.split(" =", 1) for ln in run.stdout.splitlines() if " =" in ln)
    arr = lambda k: np.array([float(v) for v in kv[k].split()])
    x = arr("x")          # the pose vector the driver's calls ran at, exactly
    with aar.Problem(ds) as p:
        lev, rows, _ = p.track_smooth_detection_leverage(x, SROT, STRANS, frame_time=ft, rows=True, **kw)
        loo = p.track_smooth_detection_loo(x, SROT, STRANS, frame_time=ft, f_max=2.5, **kw)
        uv, cov, st, _, _ = p.track_smooth_predict_corners(x, SROT, STRANS, qc, qm, qt, frame_time=ft, **kw)
        inn, m2, _, _, _ = p.track_smooth_gate_detections(x, SROT, STRANS, qc, qm, qt, arr("obs"), frame_time=ft, **kw)
    assert np.array_equal(arr("leverage"), lev) and np.array_equal(arr("rows"), rows.reshape(-1))
    assert np.array_equal(arr("F"), loo.F, equal_nan=True) and np.array_equal(arr("q"), loo.q, equal_nan=True) and np.array_equal(arr("keep"), loo.keep)
    assert [int(kv[k]) for k in ("rejected", "undetermined", "argmax_f", "launches")] == [loo.report[k] for k in ("rejected", "undetermined", "argmax_f", "launches")]
    assert float(kv["sigma2"]) == loo.report["sigma2"] and 0 < loo.report["rejected"] < ds.num_obs
    assert np.array_equal(arr("uv"), uv.reshape(-1)) and np.array_equal(arr("cov"), cov.reshape(-1)) and np.array_equal(arr("status"), st)
    assert np.array_equal(arr("innovation"), inn.reshape(-1)) and np.array_equal(arr("m2"), m2)
    assert "no camera with id %d" % (1 << 20) in kv["bad_id"]


@pytest.mark.parametrize("model", MODELS)
def test_find_solution_smooth_loo_switches(tmp_path, model):
    import os
    import subprocess
    from conftest import PKG
    from test_loo_layers_host import parse_loo_yaml
    P = sl.PLANT
    ds, x0, i = sl.planted()
    ds.x_full = x0
    ds.x_truth = None
    triple = (int(ds.frame_ids[ds.obs_frame[i]]), int(ds.cam_ids[ds.obs_cam[i]]), int(ds.marker_ids[ds.obs_marker[i]]))
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    os.mkdir(folder)
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), ds)
    kw = sl.PLANT_MODELS[model]
    base = [exe, folder, str(ds.marker_size), "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    smooth = ["-smooth", repr(P["sigma_rot"]), repr(P["sigma_trans"])] + (["-cv", repr(kw["sigma_rot0"]), repr(kw["sigma_trans0"])] if model == "cv" else [])
    env = dict(os.environ, AAR_DETERMINISTIC="1")
    path = os.path.join(folder, "final.smooth_loo.yaml")
    run = subprocess.run(base + smooth + ["-smooth-loo", str(sl.PLANT_F_MAX)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert len([l for l in run.stdout.splitlines() if l.startswith("smooth-loo: ")]) == 1, run.stdout
    y = parse_loo_yaml(path)
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    assert got.num_obs == ds.num_obs
    with aar.Problem(got) as p:
        loo = p.track_smooth_detection_loo(got.x_full, P["sigma_rot"], P["sigma_trans"], frame_time=np.asarray(got.frame_ids, dtype=np.float64),
                                           f_max=sl.PLANT_F_MAX, **kw)
    # (the solution file stores Rodrigues(matrix) of every pose, a few ulps from the driver's own vector: the figures agree closely, not to the bit)
    rep = loo.report
    assert y["f_max"] == sl.PLANT_F_MAX and y["dof"] == rep["dof"] == 8 * ds.num_obs - 6 and y["rejected"] == rep["rejected"] and y["undetermined"] == 0
    np.testing.assert_allclose([y["sigma2"], y["max_f"], y["leverage_sum"]], [rep["sigma2"], rep["max_f"], rep["leverage_sum"]], rtol=1e-6)
    want = np.nonzero(loo.keep == 0)[0]
    assert [r[:3] for r in y["listed"]][0] == triple and len(y["listed"]) == len(want)
    np.testing.assert_allclose([r[3] for r in y["listed"]], loo.F[want], rtol=1e-6)
    assert max(r[3] for r in y["listed"]) == y["listed"][0][3]          # the planted detection carries the largest F
    for k, c in enumerate(got.cam_ids):
        sel = np.asarray(got.obs_cam) == k
        n, mx, rej = y["cameras"][int(c)]
        assert n == sel.sum() and rej == int((loo.keep[sel] == 0).sum())
    # -smooth-reject-loo: round one drops the planted detection, one detection per frame and round, and the smoother runs again
    os.remove(path)
    run = subprocess.run(base + smooth + ["-smooth-reject-loo", str(sl.PLANT_F_MAX)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    rounds = [l for l in run.stdout.splitlines() if l.startswith("smooth-reject-loo round ")]
    assert 1 <= len(rounds) <= 3 and rounds[0].endswith(" 1 detections dropped") and not os.path.exists(path), run.stdout
    left = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    remaining = set(zip(np.asarray(left.frame_ids)[left.obs_frame].tolist(), np.asarray(left.cam_ids)[left.obs_cam].tolist(),
                        np.asarray(left.marker_ids)[left.obs_marker].tolist()))
    assert triple not in remaining and left.num_obs < ds.num_obs
    # refused with the usage message: without -smooth, with -with-huber, without a value
    for bad in (base + ["-smooth-loo", "3"], base + smooth + ["-with-huber", "-smooth-loo", "3"], base + smooth + ["-smooth-reject-loo"],
                base + smooth + ["-smooth-loo", "-1"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-smooth-loo" in run.stdout and "smooth-loo: " not in run.stdout, run.stdout
