"""The CPU checker against the golden vectors (and against the live reference solver where it is built).

Pins oracle/ba_oracle.cpp -- the restated LM loop, J^T J product and sparse LDL^T -- to outputs of the REAL
ucoslam::SparseLevMarq<double> / Eigen::SimplicialLDLT (tests/golden/make_golden.py, tests/golden/make_ref_vectors.py).  CPU only.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle_lib as ol
from conftest import GOLDEN, load_golden

G1 = ["g1_cfg2", "g1_cfg3_cut", "g1_cfg2_far", "g1_cfg2_retry"]


@pytest.mark.parametrize("name", G1)
def test_residual_rows_match_golden(name):
    ds, g = load_golden(name)
    o = ol.Oracle(ds)
    assert np.array_equal(o.residuals(ds.x_full, res_mode=ol.RES_F32), g["r0_f32"])  # bit-exact


@pytest.mark.parametrize("name", G1)
@pytest.mark.parametrize("flavour,jm", [("faithful_", ol.JAC_NUMERIC_F32), ("analytic_", ol.JAC_ANALYTIC)])
def test_port_lm_reproduces_real_solver_trace(name, flavour, jm):
    ds, g = load_golden(name)
    o = ol.Oracle(ds)
    tau = float(g["tau"][0]) if "tau" in g else 1.0
    x, rep = o.lm_solve(ds.x_full, params=ol.mapper_params(tau=tau), jac_mode=jm, res_mode=ol.RES_F32, threads=2)
    err = np.array([t["err"] for t in rep["trace"]])
    mu = np.array([t["mu"] for t in rep["trace"]])
    st = o.reproj_stats(x)
    if name == "g1_cfg2_retry":
        # tau = 1e-6 makes (JtJ + mu I) nearly singular on the first steps: two exact solvers (this LDL^T with a
        # frames-first order, Eigen's with AMD) differ at 1e-6 relative there and the paths separate slightly
        # before meeting at the same minimum.  The retry branch itself is what this case is for.
        assert abs(rep["iterations"] - int(g[flavour + "iterations"][0])) <= 2
        np.testing.assert_allclose(err[:4], g[flavour + "err"][:4], rtol=1e-6)
        assert max(t["tries"] for t in rep["trace"]) > 1
        assert abs(st["rmse"] - g[flavour + "rmse"][0]) < 1e-5
        return
    assert rep["iterations"] == int(g[flavour + "iterations"][0])
    np.testing.assert_allclose(err, g[flavour + "err"], rtol=1e-7)   # two exact sparse LDL^T orders
    np.testing.assert_allclose(mu, g[flavour + "mu"], rtol=1e-6)
    np.testing.assert_allclose(x, g[flavour + "x"], atol=1e-7)
    assert abs(st["rmse"] - g[flavour + "rmse"][0]) < 1e-9


def test_faithful_and_analytic_agree_below_the_parity_bar():
    # the numeric float Jacobian and the analytic one stop at the same reprojection error
    for name in G1:
        _, g = load_golden(name)
        assert abs(g["faithful_rmse"][0] - g["analytic_rmse"][0]) < 1e-5


@pytest.mark.parametrize("flavour,jm,rm", [("faithful_", ol.JAC_NUMERIC_F32, ol.RES_F32), ("analytic_", ol.JAC_ANALYTIC, ol.RES_F64)])
def test_normal_equations_and_ldlt_match_eigen(flavour, jm, rm):
    ds, g = load_golden("g2_small")
    o = ol.Oracle(ds)
    rows, cols, vals = o.jacobian(ds.x_full, jac_mode=jm)
    J = sp.coo_matrix((vals, (rows, cols)), shape=(8 * o.N, o.num_vars)).tocsr()
    Jg = sp.coo_matrix((g[flavour + "J_vals"], (g[flavour + "J_rows"], g[flavour + "J_cols"])), shape=J.shape).tocsr()
    assert abs(J - Jg).max() == 0.0  # same Jacobian entries
    H, B = o.normal_equations(ds.x_full, jac_mode=jm, res_mode=rm)
    scale = np.abs(g[flavour + "JtJ"]).max()
    assert np.abs(H - g[flavour + "JtJ"]).max() / scale < 1e-13       # restated mult() vs Eigen Jt*J
    np.testing.assert_allclose(B, g[flavour + "B"], rtol=1e-12, atol=1e-9 * np.abs(B).max())
    for mu, dref in zip(g[flavour + "mu"], g[flavour + "delta"]):
        d = o.damped_solve(ds.x_full, float(mu), jac_mode=jm, res_mode=rm)
        assert np.abs(d - dref).max() / np.abs(dref).max() < 1e-8     # own sparse LDL^T vs SimplicialLDLT


def test_analytic_jacobian_matches_central_differences():
    ds, _ = load_golden("g1_cfg2")
    o = ol.Oracle(ds)
    shp = (8 * o.N, o.num_vars)
    Ja = sp.coo_matrix((lambda t: (t[2], (t[0], t[1])))(o.jacobian(ds.x_full, jac_mode=ol.JAC_ANALYTIC)), shape=shp).toarray()
    Jn = sp.coo_matrix((lambda t: (t[2], (t[0], t[1])))(o.jacobian(ds.x_full, jac_mode=ol.JAC_NUMERIC_F64)), shape=shp).toarray()
    assert np.abs(Ja - Jn).max() < 5e-6 * max(1.0, np.abs(Ja).max() / 1e3)
    # reference-faithful float Jacobian: quantisation noise of about ulp(proj)/2e-3 per entry
    Jf = sp.coo_matrix((lambda t: (t[2], (t[0], t[1])))(o.jacobian(ds.x_full, jac_mode=ol.JAC_NUMERIC_F32)), shape=shp).toarray()
    assert np.abs(Ja - Jf).max() < 0.2


def test_fixed_groups_shrink_the_parameter_vector():
    ds, _ = load_golden("g2_small")
    full = ol.Oracle(ds)
    for opt in [(True, False, True), (False, True, True), (True, True, False), (False, False, True)]:
        o = ol.Oracle(ds, optimize=opt)
        exp = (6 * (ds.num_cams - 1) if opt[0] else 0) + (6 * (ds.num_markers - 1) if opt[1] else 0) + (6 * ds.num_frames if opt[2] else 0)
        assert o.num_vars == exp
        z = o.extract_z(ds.x_full)
        assert np.array_equal(o.merge_z(ds.x_full, z), ds.x_full)
        assert np.array_equal(o.residuals(ds.x_full), full.residuals(ds.x_full))


def test_rodrigues_restatement():
    rng = np.random.default_rng(7)
    for _ in range(200):
        w = rng.normal(size=3)
        w *= rng.uniform(0, 3.0) / np.linalg.norm(w)
        R = ol.rodrigues_vec2mat(w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        np.testing.assert_allclose(ol.rodrigues_mat2vec(R), w, atol=1e-12)
    # theta below DBL_EPSILON -> identity (cv::Rodrigues)
    assert np.array_equal(ol.rodrigues_vec2mat(np.array([1e-17, 0, 0])), np.eye(3))
    # theta = pi branch (SURVEY.md section 8d caution): the axis comes from the diagonal
    for axis in (np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([1.0, 2.0, -2.0]) / 3.0):
        w = axis * np.pi
        R = ol.rodrigues_vec2mat(w)
        w2 = ol.rodrigues_mat2vec(R)
        assert min(np.abs(w2 - w).max(), np.abs(w2 + w).max()) < 1e-7
        np.testing.assert_allclose(ol.rodrigues_vec2mat(w2), R, atol=1e-10)
    # a slightly non-orthogonal input is projected onto SO(3) first
    R = ol.rodrigues_vec2mat(np.array([0.3, -0.2, 0.5]))
    np.testing.assert_allclose(ol.rodrigues_mat2vec(R * (1 + 1e-6)), [0.3, -0.2, 0.5], atol=1e-9)


def test_port_lm_with_huber_schedule_matches_real_solver():
    # -with-huber: hubberDelta = 10 at the start of solve(), lowered by 7.5/500 after every step down to 2.5
    # (libs/multicam_mapper.cpp:412-417,425); the changing delta keeps the solver running for ~500 steps
    ds, g = load_golden("g1_cfg2_huber")
    o = ol.Oracle(ds, with_huber=True)
    x, rep = o.lm_solve(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32, threads=2)
    assert rep["iterations"] == int(g["analytic_iterations"][0]) == 505
    err = np.array([t["err"] for t in rep["trace"]])
    np.testing.assert_allclose(err, g["analytic_err"], rtol=1e-5)
    np.testing.assert_allclose(x, g["analytic_x"], atol=1e-4)
    assert abs(o.reproj_stats(x)["rmse"] - g["faithful_rmse"][0]) < 1e-4
    # the outliers are down-weighted: the unweighted optimum is pulled away from where the Huber one sits
    plain_x, _ = ol.Oracle(ds).lm_solve(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32, threads=2)
    assert np.abs(plain_x - x).max() > 1e-3


@pytest.mark.parametrize("name", ["g_track_cfg2", "g_track_cfg2_huber"])
def test_track_port_matches_real_solver_autodiff(name):
    # track(): the restated calcDerivates (central differences, der_epsilon 1e-3, |d| <= 1e-4 dropped) + LM loop against the
    # golden produced by the real solver's own solve(z, f) (libs/sparselevmarq.h:165-228)
    ds, g = load_golden(name)
    hub = bool(g["with_huber"][0])
    x, it, err = ol.track_frames(ds, g["track_x0"], with_huber=hub, huber_delta=10.0)
    assert np.array_equal(it, g["track_iterations"])
    np.testing.assert_allclose(err, g["track_err"], rtol=1e-9)
    np.testing.assert_allclose(x, g["track_x"], atol=1e-10)
    ns = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    assert np.array_equal(x[:ns], g["track_x0"][:ns])


def test_huber_weight_restatement():
    # libs/multicam_mapper.cpp:11-24,1014-1019: rows scaled by sqrt(rho(e)/e); inliers untouched
    ds, _ = load_golden("g2_small")
    plain = ol.Oracle(ds).residuals(ds.x_full)
    e = (plain.reshape(-1, 2) ** 2).sum(1)
    delta = float(np.float32(np.sqrt(np.median(e))))  # splits the corners into inliers and outliers
    hub = ol.Oracle(ds, with_huber=True, huber_delta=delta).residuals(ds.x_full)
    d2 = float(np.float32(delta) * np.float32(delta))
    w = np.where(e <= d2, 1.0, np.sqrt((2 * delta * np.sqrt(e) - d2) / np.maximum(e, 1e-300)))
    np.testing.assert_allclose(hub.reshape(-1, 2), plain.reshape(-1, 2) * w[:, None], rtol=1e-6)
    assert (w < 1).any() and (w == 1).any()


def test_port_equals_live_reference_solver():
    # the real solver's result of this very call is stored (tests/golden/make_ref_vectors.py); where oracle/_ref is built, the live solver must still give it
    ds, _ = load_golden("g1_cfg3_cut")
    g = np.load(os.path.join(GOLDEN, "g1_cfg3_cut_ref_threads2.npz"))
    r2 = {"iterations": int(g["iterations"][0]), "final_err": float(g["final_err"][0])}
    x2 = g["x"]
    o = ol.Oracle(ds)
    if ol.have_ref():
        xl, rl = o.ref_lm_solve(ds.x_full, threads=2)
        assert rl["iterations"] == r2["iterations"]
        np.testing.assert_allclose(rl["final_err"], r2["final_err"], rtol=1e-10)
        np.testing.assert_allclose(xl, x2, atol=1e-9)
    x1, r1 = o.lm_solve(ds.x_full, threads=2)
    assert r1["iterations"] == r2["iterations"]
    np.testing.assert_allclose(r1["final_err"], r2["final_err"], rtol=1e-10)
    np.testing.assert_allclose(x1, x2, atol=1e-9)


def test_intrinsics_block_restatement_matches_real_solver():
    # optimize_cam_intrinsics (libs/multicam_mapper.cpp:488-498,580-593,788-798,835-893): z ends with fx cx fy cy d0..d4 per
    # camera (root included); the port's LM must reproduce the real solver's trace for both Jacobian flavours, the analytic
    # intrinsics columns must equal central differences, and the five distortion columns are exact zeros
    ds, g = load_golden("g1_cfg2_intr")
    o = ol.Oracle(ds, intrinsics=True)
    assert o.num_vars == ds.full_len + 9 * ds.num_cams
    z = o.extract_z(ds.x_full)
    i0 = ds.full_len
    K = ds.cam_mats.reshape(-1, 9)
    np.testing.assert_array_equal(z[i0:].reshape(-1, 9)[:, :4], np.stack([K[:, 0], K[:, 2], K[:, 4], K[:, 5]], axis=1))   # fx cx fy cy (:488-498)
    np.testing.assert_array_equal(z[i0:].reshape(-1, 9)[:, 4:], ds.dist_coeffs)
    assert np.array_equal(o.residuals(ds.x_full, z, res_mode=ol.RES_F32), g["r0_f32"])
    # the skew of the calibration (0.4 here) does not survive intrinsics_vec2mats: rows differ from the fixed-intrinsics rows
    assert not np.array_equal(ol.Oracle(ds).residuals(ds.x_full, res_mode=ol.RES_F32), g["r0_f32"])
    import scipy.sparse as sp
    Ja = sp.coo_matrix((lambda t: (t[2], (t[0], t[1])))(o.jacobian(ds.x_full, z, jac_mode=ol.JAC_ANALYTIC)), shape=(8 * o.N, o.num_vars)).toarray()
    Jn = sp.coo_matrix((lambda t: (t[2], (t[0], t[1])))(o.jacobian(ds.x_full, z, jac_mode=ol.JAC_NUMERIC_F64)), shape=(8 * o.N, o.num_vars)).toarray()
    assert np.abs(Ja - Jn).max() < 1e-6 * np.abs(Ja).max()
    assert np.abs(Ja[:, i0:]).max() > 0 and not Ja[:, i0:].reshape(8 * o.N, -1, 9)[:, :, 4:].any()
    for jm, tag in ((ol.JAC_ANALYTIC, "analytic_"), (ol.JAC_NUMERIC_F32, "faithful_")):
        x, rep = o.lm_solve(ds.x_full, jac_mode=jm, res_mode=ol.RES_F32)
        assert rep["iterations"] == int(g[tag + "iterations"][0])
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], g[tag + "err"], rtol=1e-6)
        np.testing.assert_allclose(rep["z"], g[tag + "z"], atol=1e-5)
        assert np.array_equal(rep["z"][i0:].reshape(-1, 9)[:, 4:], ds.dist_coeffs)      # the distortion entries never move
    # the float-quantised central differences hurt here (a column of x/w ~ 0.3 with 0.02 of quantisation noise): the
    # reference's own run stops 3e-4 px above the optimum the analytic Jacobian reaches
    assert 0 < g["faithful_rmse"][0] - g["analytic_rmse"][0] < 1e-3
