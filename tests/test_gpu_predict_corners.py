"""aar_problem_predict_corners and aar_problem_detection_leverage on the device (csrc/predict_kernels.hip) against the
float64 restatement of tests/predict_restated.py.  Needs a real MI355X.  Every problem is created with solver="direct", deterministic=True
and runs at ds.x_full.  A case is run ONCE (_run): the device's dense normal equations, its dense covariance, one predict_corners call on
every detection plus every (camera, marker) of three frames, one detection_leverage call; the tests share that record.

Certificate (test_certificate).  C_ref is built in float64 from what the DEVICE returns -- entity_cov and the frame blocks of
Problem.covariance(dense=True), the gains G_a^(f) = V_f^-1 W_a^T from the device's eval_normal_equations, the complex-step J of
tests/projection_reference.py -- so that the error of the covariance chain (DESIGN.md sections 13, 21) is not charged twice.  Per query

    |C_dev - C_ref|_F <= gamma_q kappa_f s_q + 2 SCALED_BAR s_q        s_q = | |J| |Sigma_q| |J^T| |_F,  kappa_f = cond_2(V_f)
    gamma_q = (6 k_f + 18 + 36) 2^-53

gamma_q is an operation count of k_predict_corners as written: an entry of Sigma_fe is a sum of 6 k_f products in slot order (k_f the
frame's slots); every gain entry is a six-term sum with V_f^-1 (6), whose own elimination costs at most 2 * 6 operations per entry (12),
relative to kappa_f; T = G Sigma and C = T G^T are 18-term sums (36).  SCALED_BAR is the project's measured agreement between the closed-form
and the complex-step Jacobian; J enters C twice.  MEASURED worst ratio per case (MI355X, ROCm 7):

    sweep2 3.1e-5   gauge_c16 3.3e-5   cams_off_3 5.4e-5   markers_off_3 2.2e-5   fixed_3 4.2e-5   worklist_unseen 6.2e-5   empty_frame 4.6e-5
    roots_only_frame 5.0e-5   small_frames 2.3e-5   wide_84 4.3e-5   huber 6.3e-5   priors_fixed 5.2e-5   g2_small 7.4e-4

The ratios are small because SCALED_BAR (5e-12) dominates the bar and the kernel's own rounding is a few 2^-53 of s_q: the bar's first term,
the one an error of the slot sum or of a product would have to stay under, is 1e-14 .. 1e-12 of s_q (kappa_f 30 .. 13 000).

End to end (test_end_to_end): against numpy.linalg.inv of the device's dense H, |C_dev - C_ref|_F <= 1e-7 s_q, on the cases whose two float64
routes stay below 1/8 of that bar on the host (tests/test_predict_restated_host.py: all but g2_small, which the certificate covers).
Measured: 8e-14 (cams_off_3) .. 1.8e-12 (small_frames), 3.7e-11 on huber.
"""
import ctypes as C

import numpy as np
import pytest

import aar
import predict_restated as prs
from conftest import load_golden
from covariance_cases import CASES, case_keywords, fixed_of
from reduced_system import prior_terms
from test_predict_restated_host import FLAT_CASES, NAMES

pytestmark = pytest.mark.gpu

ROW_BAR = 1e-9             # the project's bar for double-mode rows, in pixels (tests/test_gpu_observation_passes.py)
_RUNS = {}
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_report():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")
    yield
    print("\npredicted corners: worst certificate ratio, worst end-to-end |C_dev - C_ref| / s_q per case")
    for name, v in sorted(RATIOS.items()):
        print("  %-18s %s" % (name, "  ".join("%s %.3e" % kv for kv in sorted(v.items()))))


def _case(name):
    make, kw = CASES[name]
    ds = make()
    opt, intr, hub, fixed, pri = case_keywords(ds, kw, np.asarray(ds.x_full, dtype=np.float64))
    assert not intr
    pk = dict(optimize=opt, with_huber=hub, solver="direct", deterministic=True, **fixed)
    if pri:
        pk["priors"] = pri
    return ds, pk, opt, fixed, pri


class Run:
    pass


def _run(name):
    """the shared record of a case (kept for the module: a few MB each)"""
    if name in _RUNS:
        return _RUNS[name]
    r = Run()
    r.ds, r.pk, r.opt, r.fixed, r.pri = _case(name)
    r.x = np.asarray(r.ds.x_full, dtype=np.float64)
    r.nd = int(r.ds.num_obs)
    r.q = np.concatenate([prs.detection_queries(r.ds), prs.frame_grid_queries(r.ds, prs.three_frames(r.ds))])
    with aar.Problem(r.ds, **r.pk) as p:
        r.H, _, r.ss = p.eval_normal_equations(r.x)          # (the device's H carries the priors' blocks)
        r.cv = p.covariance(r.x, dense=True)
        r.uv, r.cov, r.st, r.rep = p.predict_corners(r.x, r.q)
        r.lev, r.rows, r.lrep = p.detection_leverage(r.x, rows=True)
        r.cv_after = p.covariance(r.x, dense=True)
        r.num_vars = p.num_vars
    r.ps = prs.PredictSystem(r.ds, r.H, r.opt, **r.fixed)
    r.uv_ref, r.J, r.depth = prs.query_projection(r.ds, r.x, r.q)
    r.st_ref = r.ps.status(r.q, r.depth)
    _RUNS[name] = r
    return r


def _dense(r):
    """(C, s, uv, status) of the record's queries by the dense route on the device's H, computed once"""
    if not hasattr(r, "dense"):
        r.dense = prs.covariances(r.ps, r.x, r.q, "dense")
    return r.dense


def _ratio(Cdev, Cref, scale):
    ok = np.isfinite(scale)
    assert np.array_equal(np.isnan(Cdev), np.isnan(Cref))
    if not ok.any():
        return np.zeros(0)
    d, sc = np.linalg.norm((Cdev - Cref)[ok], axis=(1, 2)), scale[ok]
    # (a triple of constants has Sigma_q = 0: scale 0, and then the device must give exactly 0)
    return np.where(sc > 0, d / np.where(sc > 0, sc, 1.0), np.where(d > 0, np.inf, 0.0))


# ---- 5. certificate ----
@pytest.mark.parametrize("name", NAMES)
def test_certificate(name):
    r = _run(name)
    assert np.array_equal(r.st, r.st_ref)
    ref = prs.with_device_blocks(r.ps, r.cv.entity_cov, r.cv.frames if r.cv.frames is not None else np.zeros((0, 6, 6)))
    Cref, s, _, _ = prs.covariances(ref, r.x, r.q)
    bars = prs.certificate_bars(r.ps, r.q, s)
    ratio = _ratio(r.cov, Cref, bars)
    flat = _ratio(r.cov, Cref, s)
    print("%s: %d queries, worst |C_dev - C_ref| / bar = %.3e (median %.3e), worst / s_q = %.3e" % (name, len(r.q), ratio.max(), np.median(ratio), flat.max()))
    RATIOS.setdefault(name, {})["certificate"] = float(ratio.max())
    assert ratio.max() <= 1.0, (name, float(ratio.max()))


# ---- 6. end to end ----
@pytest.mark.parametrize("name", FLAT_CASES)
def test_end_to_end(name):
    r = _run(name)
    Cref, s, _, st = _dense(r)
    assert np.array_equal(r.st, st)
    ratio = _ratio(r.cov, Cref, s)
    print("%s: worst |C_dev - C_dense| / s_q = %.3e" % (name, ratio.max()))
    RATIOS.setdefault(name, {})["end_to_end"] = float(ratio.max())
    assert ratio.max() <= prs.FLAT_BAR, (name, float(ratio.max()))
    # the report is the covariance call's
    assert r.rep["num_vars"] == r.num_vars and r.rep["num_residuals"] == 8 * r.nd
    np.testing.assert_allclose([r.rep["sum_sq"], r.rep["sigma2"]], [r.cv.sum_sq, r.cv.sigma2], rtol=1e-12)
    assert r.rep["num_live_vars"] == r.ps.num_live_vars and r.rep["launches"] > 0 and r.rep["seconds"] > 0


# ---- 7. projection ----
@pytest.mark.parametrize("name", ["sweep2", "fixed_3", "g2_small"])
def test_projection(name):
    r = _run(name)
    fin = (r.st & prs.BEHIND) == 0
    assert fin.all()
    d = np.abs(r.uv.reshape(-1, 8) - r.uv_ref).max()
    print("%s: uv against the float64 forward model: %.3e px" % (name, d))
    assert d <= ROW_BAR
    with aar.Problem(r.ds, residual_mode=aar.RES_F64, **{k: v for k, v in r.pk.items() if k != "with_huber"}) as p:
        res, _ = p.eval_residuals(r.x)
        uv2, cov2, st2, rep2 = p.predict_corners(r.x, r.q, covariance=False)
        uv3, _, st3, _ = p.predict_corners(r.x, r.q)
    obs = np.asarray(r.ds.obs_uv, dtype=np.float32).reshape(-1, 8).astype(np.float64)
    d = np.abs(r.uv[:r.nd].reshape(-1, 8) - (obs - res.reshape(-1, 8))).max()
    print("%s: uv of the detections against observed - residual: %.3e px" % (name, d))
    assert d <= ROW_BAR
    # cov = NULL: no covariance chain, the same bits
    assert cov2 is None and np.array_equal(uv2, uv3) and np.array_equal(st2, st3) and np.array_equal(uv2, r.uv) and np.array_equal(st2, r.st)
    assert rep2["launches"] == 2 and np.isnan(rep2["sigma2"]) and rep2["num_live_vars"] == r.rep["num_live_vars"]


# ---- 8. masks and status ----
@pytest.mark.parametrize("name,kind", [("sweep2", "roots"), ("fixed_3", "fixed"), ("cams_off_3", "cams"), ("markers_off_3", "markers")])
def test_constants_contribute_zero_not_nan(name, kind):
    r = _run(name)
    ds = r.ds
    if kind == "roots":
        sels = [(r.q[:, 0] == ds.root_cam, 0), (r.q[:, 1] == ds.root_marker, 1)]
    elif kind == "fixed":
        fx = fixed_of(ds)
        sels = [(np.isin(r.q[:, 0], fx["fixed_cams"]), 0), (np.isin(r.q[:, 1], fx["fixed_markers"]), 1)]
    else:
        sels = [(np.ones(len(r.q), bool), 0 if kind == "cams" else 1)]
    Cref, s, _, _ = _dense(r)
    for sel, g in sels:
        sel = sel & (r.st == 0)
        assert sel.sum() >= 4
        assert np.isfinite(r.cov[sel]).all()
        # the reference is the formula with that block zero ...
        for i in np.nonzero(sel)[0][:8]:
            S = r.ps.sigma_dense(*[int(v) for v in r.q[i]])
            assert not S[6 * g:6 * g + 6].any() and not S[:, 6 * g:6 * g + 6].any() and S.any()
        # ... and the device agrees with it
        assert _ratio(r.cov[sel], Cref[sel], s[sel]).max() <= prs.FLAT_BAR


def test_unseen_marker_and_empty_frame_are_undefined():
    r = _run("worklist_unseen")
    sel = r.q[:, 1] == 7
    assert sel.sum() >= r.ds.num_cams
    assert ((r.st[sel] & prs.UNDEFINED) != 0).all() and np.isnan(r.cov[sel]).all() and np.isfinite(r.uv[sel & ((r.st & prs.BEHIND) == 0)]).all()
    assert (r.st[~sel] == 0).all() and np.isfinite(r.cov[~sel]).all()
    assert r.rep["undefined"] == sel.sum() and r.rep["behind"] == 0
    e = _run("empty_frame")
    q = prs.frame_grid_queries(e.ds, [5, 4])
    with aar.Problem(e.ds, **e.pk) as p:
        uv, cov, st, rep = p.predict_corners(e.x, q)
    f5 = q[:, 2] == 5
    assert ((st[f5] & prs.UNDEFINED) != 0).all() and np.isnan(cov[f5]).all() and np.isfinite(uv[f5]).all()
    assert (st[~f5] == 0).all() and np.isfinite(cov[~f5]).all() and rep["undefined"] == f5.sum()


def test_a_camera_that_looks_away_is_behind():
    r = _run("sweep2")
    ds = r.ds
    f = 3
    x = r.x.copy()
    o = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1) + 6 * f
    Rx = np.diag([1.0, -1.0, -1.0])                                  # the frame pose turned by pi about x: the object lies behind the root camera
    x[o:o + 3] = aar.rodrigues_mat2vec(Rx @ aar.rodrigues_vec2mat(x[o:o + 3]))
    x[o + 3:o + 6] = Rx @ x[o + 3:o + 6]
    q = np.array([[ds.root_cam, m, f] for m in range(ds.num_markers)] + [[ds.root_cam, 0, f + 1]])
    _, _, depth = prs.query_projection(ds, x, q)
    assert (depth[:-1] < 0).all() and (depth[-1] > 0).all()
    with aar.Problem(ds, **r.pk) as p:
        for covariance in (False, True):
            uv, cov, st, rep = p.predict_corners(x, q, covariance=covariance)
            assert ((st[:-1] & prs.BEHIND) != 0).all() and st[-1] == 0
            assert np.isnan(uv[:-1]).all() and np.isfinite(uv[-1]).all()
            assert rep["behind"] == len(q) - 1 and rep["undefined"] == 0
            if covariance:
                assert np.isnan(cov[:-1]).all() and np.isfinite(cov[-1]).all()


def test_frames_as_constants():
    # a problem that does not optimise the frames: Sigma_ff = Sigma_fe = 0, the kernel touches neither V^-1 nor W nor the gains
    make, _ = CASES["sweep2"]
    ds = make()
    x = np.asarray(ds.x_full, dtype=np.float64)
    opt = (True, True, False)
    q = np.concatenate([prs.detection_queries(ds), prs.frame_grid_queries(ds, prs.three_frames(ds))])
    with aar.Problem(ds, optimize=opt, solver="direct", deterministic=True) as p:
        H, _, _ = p.eval_normal_equations(x)
        uv, cov, st, rep = p.predict_corners(x, q)
        lev, rows, lrep = p.detection_leverage(x, rows=True)
    ps = prs.PredictSystem(ds, H, opt)
    Cref, s, uv_ref, st_ref = prs.covariances(ps, x, q, "dense")
    assert np.array_equal(st, st_ref) and (st == 0).all() and ps.frame_state(0) == ("const",)
    ratio = _ratio(cov, Cref, s)
    print("frames as constants: worst |C_dev - C_dense| / s_q = %.3e, sum of leverages %.10f, P_live %d" % (ratio.max(), lev.sum(), ps.num_live_vars))
    assert ratio.max() <= prs.FLAT_BAR and np.abs(uv.reshape(-1, 8) - uv_ref).max() <= ROW_BAR
    nd = ds.num_obs
    assert np.array_equal(lev, prs.trace_tree(cov[:nd])) and np.array_equal(rows, np.diagonal(cov[:nd], axis1=1, axis2=2))
    assert rep["num_live_vars"] == ps.num_live_vars == 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    assert abs(lev.sum() - ps.num_live_vars) <= prs.FLAT_BAR * s[:nd].sum()


# ---- 9. shapes ----
def test_query_counts_duplicates_and_permutations():
    r = _run("sweep2")
    rng = np.random.default_rng(9)
    with aar.Problem(r.ds, **r.pk) as p:
        for n in (1, 63, 64, 65, 257):
            idx = rng.integers(0, len(r.q), n)
            idx[n // 2] = idx[0]                                     # a duplicate
            uv, cov, st, rep = p.predict_corners(r.x, r.q[idx])
            # a query's outputs depend on its triple and the solution alone: the bits of the large call, whatever n and the neighbours
            assert np.array_equal(uv, r.uv[idx]) and np.array_equal(cov, r.cov[idx]) and np.array_equal(st, r.st[idx]), n
        perm = rng.permutation(len(r.q))
        uv, cov, st, _ = p.predict_corners(r.x, r.q[perm])
        assert np.array_equal(uv, r.uv[perm]) and np.array_equal(cov, r.cov[perm], equal_nan=True) and np.array_equal(st, r.st[perm])
        uv0, cov0, st0, rep0 = p.predict_corners(r.x, np.zeros((0, 3)))
        assert uv0.shape == (0, 4, 2) and cov0.shape == (0, 8, 8) and rep0["launches"] == 0 and rep0["undefined"] == 0
    assert np.array_equal(r.cov, r.cov.transpose(0, 2, 1), equal_nan=True)          # symmetric to the bit


@pytest.mark.parametrize("name", ["small_frames", "wide_84", "wide_92"])
def test_frames_with_one_slot_and_with_many(name):
    import direct_cases as dc
    r = _run(name)
    kf = np.array(dc.frame_entity_counts(r.ds))
    if name == "small_frames":
        assert kf.min() == 2          # (the smallest frame there is: one detection, one slot for its camera and one for its marker)
    else:
        assert kf.max() >= int(name.split("_")[1])
    # queries whose camera and marker are not among their frame's slots
    seen = set(zip(r.ds.obs_cam.tolist(), r.ds.obs_marker.tolist(), r.ds.obs_frame.tolist()))
    cams_of = {}
    mks_of = {}
    for c, m, f in seen:
        cams_of.setdefault(f, set()).add(c)
        mks_of.setdefault(f, set()).add(m)
    out = np.array([int(c) not in cams_of.get(int(f), ()) and int(m) not in mks_of.get(int(f), ()) for c, m, f in r.q])
    if name == "small_frames":
        assert (out & (r.st == 0)).sum() >= 4
    Cref, s, _, st = _dense(r)
    assert np.array_equal(r.st, st)
    ratio = _ratio(r.cov, Cref, s)
    print("%s: slots per frame %d .. %d, %d queries off their frame's slots, worst |C_dev - C_dense| / s_q = %.3e" % (name, kf.min(), kf.max(), out.sum(), ratio.max()))
    assert ratio.max() <= prs.FLAT_BAR
    assert np.array_equal(r.cov, r.cov.transpose(0, 2, 1), equal_nan=True)


# ---- 10. leverage ----
@pytest.mark.parametrize("name", NAMES)
def test_leverage(name):
    r = _run(name)
    Cd = r.cov[:r.nd]
    assert (r.st[:r.nd] == 0).all(), "a detection makes its triple seen"
    # the trace and the diagonal of predict_corners on the detection triples, to the bit
    assert np.array_equal(r.rows, np.diagonal(Cd, axis1=1, axis2=2)) and np.array_equal(r.lev, prs.trace_tree(Cd))
    total = 0.0
    for v in r.lev:
        total += v
    assert r.lrep["leverage_sum"] == total and r.lrep["undefined"] == 0 and r.lrep["behind"] == 0
    assert r.lrep["num_live_vars"] == r.ps.num_live_vars
    s = _dense(r)[1][:r.nd]
    want = float(r.ps.num_live_vars)
    if r.pri:
        Hp = prior_terms(r.ds, r.x, r.pri, r.num_vars)[0]
        want -= float(np.trace(r.ps.Hinv @ Hp[np.ix_(r.ps.idx, r.ps.idx)]))
    print("%s: sum of leverages %.12g, expected %.12g, bar %.3g; leverages %.3f .. %.3f" % (name, total, want, prs.FLAT_BAR * s.sum(), r.lev.min(), r.lev.max()))
    assert abs(total - want) <= prs.FLAT_BAR * s.sum()
    ev = np.linalg.eigvalsh(Cd)
    assert (ev.min(axis=1) >= -prs.FLAT_BAR * s).all() and (ev.max(axis=1) <= 1 + prs.FLAT_BAR * s).all()


def test_leverage_identity_at_full_size():
    ds = aar.synth(3)
    with aar.Problem(ds, solver="direct") as p:
        lev, _, rep = p.detection_leverage(ds.x_full)
    # (config 3 has markers no frame sees: their unknowns are not live)
    assert 3000 < rep["num_live_vars"] <= 3276 and rep["num_vars"] == 3276 and np.isfinite(lev).all() and lev.min() > 0 and lev.max() < 8
    # s_i >= |C_i|_F >= tr(C_i) / sqrt(8): the bar 1e-7 sum s_i is at least 1e-7 sum(leverage) / sqrt(8), which needs no reference at this size
    print("config 3: %d detections, sum of leverages %.10f, P_live %d, %.2f ms" % (len(lev), lev.sum(), rep["num_live_vars"], 1e3 * rep["seconds"]))
    assert abs(lev.sum() - rep["num_live_vars"]) <= prs.FLAT_BAR * lev.sum() / np.sqrt(8.0)
    np.testing.assert_allclose(rep["leverage_sum"], lev.sum(), rtol=1e-12)


# ---- 11. refusals ----
def _raw_predict(p, x, q, struct_size=None):
    qc, qm, qf = [np.ascontiguousarray(q[:, k], dtype=np.int32) for k in range(3)]
    uv, cov, st = np.full((len(q), 8), 7.0), np.full((len(q), 64), 7.0), np.full(len(q), 77, dtype=np.uint8)
    rep = aar.CPredictReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    code = aar.lib().aar_problem_predict_corners(p.handle, x.ctypes.data_as(dp), len(q), qc.ctypes.data_as(ip), qm.ctypes.data_as(ip), qf.ctypes.data_as(ip),
                                                 uv.ctypes.data_as(dp), cov.ctypes.data_as(dp), st.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(rep))
    untouched = np.all(uv == 7.0) and np.all(cov == 7.0) and np.all(st == 77) and bytes(bytearray(rep)[4:]) == b"\x55" * (C.sizeof(rep) - 4)
    return code, untouched


def _raw_leverage(p, x, n):
    lev, rows = np.full(max(n, 1), 7.0), np.full((max(n, 1), 8), 7.0)
    rep = aar.CPredictReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep)
    dp = C.POINTER(C.c_double)
    code = aar.lib().aar_problem_detection_leverage(p.handle, x.ctypes.data_as(dp), lev.ctypes.data_as(dp), rows.ctypes.data_as(dp), C.byref(rep))
    return code, np.all(lev == 7.0) and np.all(rows == 7.0) and bytes(bytearray(rep)[4:]) == b"\x55" * (C.sizeof(rep) - 4)


def test_refusals_leave_the_outputs_untouched():
    ds, _ = load_golden("g2_small")
    x = np.asarray(ds.x_full, dtype=np.float64)
    q = prs.detection_queries(ds)[:5]
    # a communicator (the single-rank local group of the other modules): dense outputs are single-GPU
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm, solver="direct") as p:
            for code, untouched in (_raw_predict(p, x, q), _raw_leverage(p, x, ds.num_obs)):
                assert code == aar.AAR_ERR_UNSUPPORTED and untouched
            assert "single-GPU" in aar.lib().aar_last_error().decode()
    finally:
        comm.close()
        group.close()
    # the intrinsics block
    di, _ = load_golden("g1_cfg2_intr")
    with aar.Problem(di, intrinsics=True, solver="direct") as p:
        xi = p.x_with_intrinsics(di.x_full)
        for code, untouched in (_raw_predict(p, xi, prs.detection_queries(di)[:5]), _raw_leverage(p, xi, di.num_obs)):
            assert code == aar.AAR_ERR_UNSUPPORTED and untouched
        msg = aar.lib().aar_last_error().decode()
        assert "fx, cx, fy, cy" in msg and "next step" in msg
    with aar.Problem(ds, solver="direct") as p:
        # an index out of range is named before anything runs
        bad = q.copy()
        bad[2, 1] = ds.num_markers
        code, untouched = _raw_predict(p, x, bad)
        assert code == aar.AAR_ERR_INVALID and untouched and "q_marker[2]" in aar.lib().aar_last_error().decode()
        # a pivot that is not positive passes through with aar_problem_covariance's message: a pose that is not a number
        xn = x.copy()
        m1 = [m for m in range(ds.num_markers) if m != ds.root_marker and (np.asarray(ds.obs_marker) == m).any()][0]
        o = 6 * (ds.num_cams - 1) + 6 * (m1 - (m1 > ds.root_marker))
        xn[o + 3] = np.nan
        with pytest.raises(aar.AarError) as e:
            p.covariance(xn)
        assert e.value.code == aar.AAR_ERR_NUMERIC
        want = str(e.value)
        for code, untouched in (_raw_predict(p, xn, q), _raw_leverage(p, xn, ds.num_obs)):
            assert code == aar.AAR_ERR_NUMERIC and untouched
            assert aar.lib().aar_last_error().decode() in want and "non-positive pivot" in want
        # ... and the problem works on afterwards
        uv, cov, st, _ = p.predict_corners(x, q)
        assert np.isfinite(uv).all() and (st == 0).all()


# ---- 12. unchanged behaviour ----
@pytest.mark.parametrize("name", ["sweep2", "priors_fixed"])
def test_covariance_bits_before_and_after(name):
    r = _run(name)
    assert np.array_equal(r.cv.entity_cov, r.cv_after.entity_cov, equal_nan=True) and np.array_equal(r.cv.frames, r.cv_after.frames, equal_nan=True)
    assert np.array_equal(r.cv.entity_diag_flat, r.cv_after.entity_diag_flat, equal_nan=True)
    assert (r.cv.sigma2, r.cv.min_pivot, r.cv.max_pivot) == (r.cv_after.sigma2, r.cv_after.min_pivot, r.cv_after.max_pivot)
    # two calls give the same bits, and the problem carries no LM state afterwards
    with aar.Problem(r.ds, **r.pk) as p:
        uv, cov, st, _ = p.predict_corners(r.x, r.q)
        lev, rows, _ = p.detection_leverage(r.x, rows=True)
        assert np.array_equal(uv, r.uv) and np.array_equal(cov, r.cov, equal_nan=True) and np.array_equal(st, r.st)
        assert np.array_equal(lev, r.lev) and np.array_equal(rows, r.rows)
        with pytest.raises(aar.AarError):
            p.lm_step()


# ---- the other layers ----
def test_mapper_by_id(tmp_path):
    import subprocess
    from test_predict_host import build_mapper_tool
    run = subprocess.run([build_mapper_tool(tmp_path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    kv = dict(ln.split(" = ", 1) for ln in run.stdout.splitlines() if " = " in ln)
    assert kv["queries"] == "2" and kv["status0"] == "0" and kv["uv0"] == kv["uv0_nocov"]
    assert float(kv["cov00"]) > 0 and float(kv["sigma2"]) > 0                  # (scaled by sigma2: a variance in pixels squared)
    n = int(kv["leverages"])
    assert int(kv["rows"]) == 8 * n and kv["leverage_sum"] == kv["report_sum"]
    assert abs(float(kv["leverage_sum"]) - int(kv["num_live_vars"])) <= prs.FLAT_BAR * float(kv["leverage_sum"]) / np.sqrt(8.0)


def test_find_solution_leverage_switch(tmp_path):
    # aar_find_solution -leverage h writes final.leverage.yaml beside final.solution; without the switch nothing else changes (fixed-order
    # sums, so that two solves give the same bits)
    import os
    import subprocess
    from conftest import PKG
    from test_predict_host import parse_leverage_yaml
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    env = dict(os.environ, AAR_DETERMINISTIC="1")
    got = {}
    for flag in ([], ["-leverage", "1.8"]):
        run = subprocess.run([exe, folder, "0.05", "x", "-from-initial", "-solver", "direct"] + flag, capture_output=True, text=True, timeout=300, env=env)
        assert run.returncode == 0, run.stderr
        assert os.path.exists(os.path.join(folder, "final.leverage.yaml")) == bool(flag)
        got[bool(flag)] = [open(os.path.join(folder, f), "rb").read() for f in ("final.solution", "final.solution.yaml")]
    assert got[False] == got[True]
    assert subprocess.run([exe, folder, "0.05", "x", "-leverage"], capture_output=True, text=True).returncode != 0          # (the threshold is required)
    y = parse_leverage_yaml(os.path.join(folder, "final.leverage.yaml"))
    sol = aar.solution_read(os.path.join(folder, "final.solution"))
    with aar.Problem(sol, solver="direct", deterministic=True) as p:
        lev, _, rep = p.detection_leverage(sol.x_full)
        err = p.residual_report(sol.x_full).det_err
    assert y["num_live_vars"] == rep["num_live_vars"] and y["h_min"] == 1.8
    np.testing.assert_allclose([y["sigma2"], y["leverage_sum"]], [rep["sigma2"], rep["leverage_sum"]], rtol=1e-6)
    want = np.nonzero(~(lev < 1.8))[0]
    assert len(y["listed"]) == len(want) and 0 < len(want) < len(lev)
    np.testing.assert_allclose([r[3] for r in y["listed"]], lev[want], rtol=1e-6)
    np.testing.assert_allclose([r[4] for r in y["listed"]], err[want], rtol=1e-5)
    for k, c in enumerate(sol.cam_ids):
        sel = np.asarray(sol.obs_cam) == k
        np.testing.assert_allclose(y["cameras"][int(c)], (sel.sum(), lev[sel].mean(), lev[sel].max()), rtol=1e-6)
