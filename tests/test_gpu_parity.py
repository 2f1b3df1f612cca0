"""Parity of the HIP path (through the C ABI) with the CPU oracle and the committed golden vectors.

Bars: bit-exact residual rows in reference-faithful (float) mode; <= 1e-9 px in double mode; block normal
equations <= 1e-12 relative to the oracle's J^T J of the analytic Jacobian and to Eigen's (golden G2); damped
step <= 1e-8 relative to Eigen::SimplicialLDLT; LM trace equal to the real SparseLevMarq trace driven with the
same (analytic) Jacobian; final reprojection error within 1e-4 px (north-star bar; observed ~1e-7) of the
reference-faithful CPU run.  Needs a real MI355X.
"""
import os

import numpy as np
import pytest

import aar
import oracle_lib as ol
from conftest import load_golden

pytestmark = pytest.mark.gpu


def Problem(ds, **kw):
    # This file pins the reference's STEP (Eigen::SimplicialLDLT to rounding: traces, damped steps, blocks): the direct solver, named explicitly.
    # The library's default -- solver AUTO -- is pinned in tests/test_gpu_solvers.py (final poses and errors against this path and the reference).
    kw.setdefault("solver", "direct")
    return aar.Problem(ds, **kw)

G1 = ["g1_cfg2", "g1_cfg3_cut", "g1_cfg2_far"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


@pytest.mark.parametrize("name", G1 + ["g2_small"])
def test_residual_rows(name):
    ds, g = load_golden(name)
    o = ol.Oracle(ds)
    with Problem(ds, residual_mode=aar.RES_F32) as p:
        r, ss = p.eval_residuals(ds.x_full)
        assert np.array_equal(r, o.residuals(ds.x_full, res_mode=ol.RES_F32))      # bit-exact, float-faithful
        if "r0_f32" in g:
            assert np.array_equal(r, g["r0_f32"])
        np.testing.assert_allclose(ss, float((r ** 2).sum()), rtol=1e-13)
    with Problem(ds, residual_mode=aar.RES_F64) as p:
        r, _ = p.eval_residuals(ds.x_full)
        assert np.abs(r - o.residuals(ds.x_full, res_mode=ol.RES_F64)).max() < 1e-9  # px


def test_block_normal_equations_vs_eigen_golden():
    ds, g = load_golden("g2_small")
    with Problem(ds, residual_mode=aar.RES_F64) as p:
        H, B, ss = p.eval_normal_equations(ds.x_full)
        scale = np.abs(g["analytic_JtJ"]).max()
        assert np.abs(H - g["analytic_JtJ"]).max() / scale < 1e-12
        assert np.abs(H - H.T).max() == 0.0
        np.testing.assert_allclose(B, g["analytic_B"], rtol=1e-10, atol=1e-12 * np.abs(B).max())
        np.testing.assert_allclose(ss, float((g["analytic_r"] ** 2).sum()), rtol=1e-12)
        for mu, dref in zip(g["analytic_mu"], g["analytic_delta"]):
            d = p.eval_damped_step(ds.x_full, float(mu))
            assert np.abs(d - dref).max() / np.abs(dref).max() < 1e-8, mu


@pytest.mark.parametrize("name", ["g1_cfg2", "g1_cfg3_cut"])
def test_block_normal_equations_vs_oracle(name):
    ds, _ = load_golden(name)
    o = ol.Oracle(ds)
    for mode, om in ((aar.RES_F64, ol.RES_F64), (aar.RES_F32, ol.RES_F32)):
        with Problem(ds, residual_mode=mode) as p:
            H, B, _ = p.eval_normal_equations(ds.x_full)
            Ho, Bo = o.normal_equations(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=om)
            assert np.abs(H - Ho).max() / np.abs(Ho).max() < 1e-12
            assert np.abs(B - Bo).max() / np.abs(Bo).max() < 1e-11
            # against the reference-faithful numeric Jacobian: equal up to its float quantisation noise
            Hf, _ = o.normal_equations(ds.x_full, jac_mode=ol.JAC_NUMERIC_F32, res_mode=om)
            assert np.abs(H - Hf).max() / np.abs(Hf).max() < 2e-3


@pytest.mark.parametrize("opt", [(True, True, False), (True, False, True), (False, True, True), (False, False, True), (True, False, False)])
def test_fixed_parameter_groups(opt):
    # MultiCamMapper::Config with a group switched off: its columns disappear and its poses do not move
    ds, _ = load_golden("g2_small")
    o = ol.Oracle(ds, optimize=opt)
    with Problem(ds, residual_mode=aar.RES_F64, optimize=opt) as p:
        assert p.num_vars == o.num_vars
        H, B, _ = p.eval_normal_equations(ds.x_full)
        Ho, Bo = o.normal_equations(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
        assert np.abs(H - Ho).max() / np.abs(Ho).max() < 1e-12
        mu = float(np.diag(Ho).max()) * 1e-2
        d = p.eval_damped_step(ds.x_full, mu)
        do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
        assert np.abs(d - do).max() / np.abs(do).max() < 1e-8
        x, rep = p.lm_solve(ds.x_full)
        C, M = ds.num_cams, ds.num_markers
        if not opt[0]:
            assert np.array_equal(x[: 6 * (C - 1)], ds.x_full[: 6 * (C - 1)])
        if not opt[1]:
            assert np.array_equal(x[6 * (C - 1): 6 * (C - 1) + 6 * (M - 1)], ds.x_full[6 * (C - 1): 6 * (C - 1) + 6 * (M - 1)])
        if not opt[2]:
            assert np.array_equal(x[6 * (C - 1) + 6 * (M - 1):], ds.x_full[6 * (C - 1) + 6 * (M - 1):])
        assert rep["final_err"] < rep["initial_err"]


@pytest.mark.parametrize("name", G1)
def test_lm_trace_equals_real_solver_with_same_jacobian(name):
    ds, g = load_golden(name)
    with Problem(ds, residual_mode=aar.RES_F32) as p:
        x, rep = p.lm_solve(ds.x_full)
        assert rep["iterations"] == int(g["analytic_iterations"][0])
        err = np.array([t["err"] for t in rep["trace"]])
        mu = np.array([t["mu"] for t in rep["trace"]])
        np.testing.assert_allclose(err, g["analytic_err"], rtol=1e-7)
        np.testing.assert_allclose(mu, g["analytic_mu"], rtol=1e-6)
        assert all(t["tries"] == 1 and t["accepted"] == 1 for t in rep["trace"])
        np.testing.assert_allclose(x, g["analytic_x"], atol=1e-7)
        assert rep["stop_code"] == 2          # |prev-curr|/rows <= 1e-4 (libs/sparselevmarq.h:459)
        rmse, _ = p.reproj_stats(x)
        # the bar of the north star: within 1e-4 px of the reference-faithful CPU path (numeric float Jacobian)
        assert abs(rmse - g["faithful_rmse"][0]) < 1e-4
        assert abs(rmse - g["faithful_rmse"][0]) < 5e-6    # what is actually observed
        assert abs(rep["iterations"] - int(g["faithful_iterations"][0])) <= 1


def test_lm_retry_branch():
    # far start + tau = 1e-6: some first tries are rejected (mu *= v; v *= 5, libs/sparselevmarq.h:416-419)
    ds, g = load_golden("g1_cfg2_retry")
    prm = aar.lm_default_params(tau=float(g["tau"][0]))
    with Problem(ds, residual_mode=aar.RES_F32) as p:
        x, rep = p.lm_solve(ds.x_full, params=prm)
        tries = [t["tries"] for t in rep["trace"]]
        assert max(tries) > 1
        assert rep["trial_points"] == sum(tries)
        err = np.array([t["err"] for t in rep["trace"]])
        np.testing.assert_allclose(err[:4], g["analytic_err"][:4], rtol=1e-6)   # before ill-conditioning separates the paths
        assert abs(rep["iterations"] - int(g["analytic_iterations"][0])) <= 2
        rmse, _ = p.reproj_stats(x)
        assert abs(rmse - g["faithful_rmse"][0]) < 1e-4
    # Run to the numerical floor (no average-step stop rule): the loop can only end through a step whose six
    # damping tries are all rejected (step() returns false -> mustExit = 2, libs/sparselevmarq.h:419,459) or through
    # an exactly repeated error.  Which of the two, and after how many steps, depends on last-bit rounding, so the
    # checks are structural.
    ds2, g2 = load_golden("g1_cfg2")
    with Problem(ds2, residual_mode=aar.RES_F64) as p:
        x, rep = p.lm_solve(ds2.x_full, params=aar.lm_default_params(min_average_step_error_diff=0.0, max_iters=200))
        assert rep["iterations"] < 200 and rep["stop_code"] == 2
        last = rep["trace"][-1]
        errs = [rep["initial_err"]] + [t["err"] for t in rep["trace"]]
        assert all(b <= a for a, b in zip(errs[:-1], errs[1:]))
        if not last["accepted"]:
            assert last["tries"] == 6 and last["err"] == rep["trace"][-2]["err"]   # curr_z / currErr untouched
        for t in rep["trace"][:-1]:
            assert t["accepted"] == 1
        _, ss = p.eval_residuals(x, want_vector=False)
        np.testing.assert_allclose(ss, rep["final_err"], rtol=1e-13)              # the returned point is curr_z
        assert rep["final_err"] <= g2["analytic_err"][-1]   # the floor lies below where the 1e-4 stop rule halts


def test_huber_rows_and_schedule():
    # libs/multicam_mapper.cpp:11-24,1014-1019 (weights) and :412-417,425 (delta schedule driven by the step callback)
    ds, g = load_golden("g1_cfg2_huber")
    o = ol.Oracle(ds, with_huber=True, huber_delta=10.0)
    with Problem(ds, with_huber=True) as p:
        p.set_huber_delta(10.0)
        r, _ = p.eval_residuals(ds.x_full)
        assert np.array_equal(r, g["r0_f32"])                       # weighted rows, bit-exact
        p.set_huber_delta(3.25)
        r2, _ = p.eval_residuals(ds.x_full)
        o2 = ol.Oracle(ds, with_huber=True, huber_delta=3.25)
        assert np.array_equal(r2, o2.residuals(ds.x_full, res_mode=ol.RES_F32))
        assert not np.array_equal(r, r2)
        # B uses the weighted residual with the UNweighted Jacobian (the reference does not re-weight J, :976-994)
        p.set_huber_delta(10.0)
        H, B, _ = p.eval_normal_equations(ds.x_full)
        Ho, Bo = o.normal_equations(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        assert np.abs(H - Ho).max() / np.abs(Ho).max() < 1e-12
        assert np.abs(B - Bo).max() / np.abs(Bo).max() < 1e-11
        x, rep = p.lm_solve(ds.x_full, trace_cap=600)
        assert rep["iterations"] == int(g["analytic_iterations"][0])
        err = np.array([t["err"] for t in rep["trace"]])
        np.testing.assert_allclose(err, g["analytic_err"], rtol=1e-5)
        np.testing.assert_allclose(x, g["analytic_x"], atol=1e-4)
        assert abs(p.get_huber_delta() - 2.5) < 0.02                  # where optCallBack leaves it
        rmse, _ = p.reproj_stats(x)                                   # unweighted statistic
        assert abs(rmse - g["faithful_rmse"][0]) < 1e-4


@pytest.mark.parametrize("name", ["g_track_cfg2", "g_track_cfg2_huber"])
def test_track_frames_vs_real_solver(name):
    # MultiCamMapper::track(): per-frame 6-DoF LM, cameras / markers fixed; golden = the real solver's own solve(z, f)
    ds, g = load_golden(name)
    hub = bool(g["with_huber"][0])
    with Problem(ds, with_huber=hub) as p:
        if hub:
            p.set_huber_delta(10.0)            # track() sets hubberDelta = 10 and installs no schedule (:439)
        x, it, err = p.track(g["track_x0"])
        ns = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        assert np.array_equal(x[:ns], g["track_x0"][:ns])                  # cameras and markers do not move
        # analytic Jacobian vs the reference's central differences (delta 1e-3, small entries dropped): same optimum
        # (with Huber the Jacobian includes the weight's derivative, as the reference's numeric differentiation of the
        #  weighted error function does)
        np.testing.assert_allclose(err, g["track_err"], rtol=1e-5, atol=1e-6)
        assert np.abs(x[ns:] - g["track_x"][ns:]).max() < 2e-4
        assert np.abs(it - g["track_iterations"]).max() <= 1 and np.mean(it == g["track_iterations"]) > 0.9
        # against the CPU port driven with the SAME analytic Jacobian the trajectories coincide (plain residuals only:
        # the oracle's analytic Jacobian follows solve()'s convention and does not differentiate the weights)
        for f in ([] if hub else [0, ds.num_frames // 2, ds.num_frames - 1]):
            dsx = type("D", (), {})()
            dsx.__dict__.update(ds.__dict__)
            dsx.x_full = g["track_x0"]
            sub = ol.frame_subproblem(dsx, f)
            o = ol.Oracle(sub, optimize=(False, False, True), with_huber=hub, huber_delta=10.0)
            xs, rep = o.lm_solve(sub.x_full, params=ol.mapper_params(huber_fixed=1), jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
            assert rep["iterations"] == it[f]
            np.testing.assert_allclose(rep["final_err"], err[f], rtol=1e-9)
            np.testing.assert_allclose(xs[ns:ns + 6], x[ns + 6 * f: ns + 6 * f + 6], atol=1e-9)


def test_step_api_matches_solve():
    ds, g = load_golden("g1_cfg2")
    with Problem(ds) as p:
        p.lm_init(ds.x_full, aar.lm_default_params())
        its = [p.lm_step() for _ in range(3)]
        np.testing.assert_allclose([i["err"] for i in its], g["analytic_err"][:3], rtol=1e-7)
        x, err = p.lm_get_solution()
        assert err == its[-1]["err"]
        _, ss = p.eval_residuals(x, want_vector=False)
        np.testing.assert_allclose(ss, err, rtol=1e-12)


def test_known_answer_noise_free():
    # G3: no corner noise -> the optimum is the ground truth (gauge fixed by the root camera / marker)
    ds = aar.synth(2, noise_px=0.0)
    with Problem(ds, residual_mode=aar.RES_F64) as p:
        x, rep = p.lm_solve(ds.x_full, params=aar.lm_default_params(min_average_step_error_diff=1e-14))
        assert rep["final_err"] < 1e-3 * ds.num_obs   # float32-rounded detections leave ~1e-5 px of noise
        rmse, _ = p.reproj_stats(x)
        assert rmse < 1e-4
        # compare as transforms (near theta = pi two rotation vectors describe one rotation).  A few markers are seen
        # only once or twice, 25 px across: their depth/tilt valley is flat (5e-5 px for 0.02 rad), so the bar is
        # per-entity for the cameras and statistical for the rest.
        dev = np.array([max(np.abs(aar.rodrigues_vec2mat(a[:3]) - aar.rodrigues_vec2mat(b[:3])).max(), np.abs(a[3:] - b[3:]).max())
                        for a, b in zip(x.reshape(-1, 6), ds.x_truth.reshape(-1, 6))])
        assert dev[: ds.num_cams - 1].max() < 2e-4
        assert np.mean(dev < 2e-4) > 0.9 and np.median(dev) < 5e-5


def test_ragged_and_degenerate_inputs():
    ds, _ = load_golden("g1_cfg2")
    o = ol.Oracle(ds)
    # drop observations so that some frames keep a single marker observation and one keeps many
    keep = np.ones(ds.num_obs, dtype=bool)
    rng = np.random.default_rng(5)
    for f in rng.choice(ds.num_frames, 30, replace=False):
        idx = np.nonzero(ds.obs_frame == f)[0]
        keep[idx[1:]] = False
    sub = aar.Dataset.__new__(aar.Dataset)
    sub.__dict__.update(ds.__dict__)
    for k in ("obs_frame", "obs_cam", "obs_marker", "obs_uv"):
        setattr(sub, k, getattr(ds, k)[keep])
    sub.num_obs = int(keep.sum())
    os_ = ol.Oracle(sub)
    with Problem(sub, residual_mode=aar.RES_F64) as p:
        r, _ = p.eval_residuals(sub.x_full)
        assert np.abs(r - os_.residuals(sub.x_full, res_mode=ol.RES_F64)).max() < 1e-9
        H, B, _ = p.eval_normal_equations(sub.x_full)
        Ho, Bo = os_.normal_equations(sub.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
        assert np.abs(H - Ho).max() / np.abs(Ho).max() < 1e-12
        mu = float(np.diag(Ho).max())
        d = p.eval_damped_step(sub.x_full, mu)
        do = os_.damped_solve(sub.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
        assert np.abs(d - do).max() / np.abs(do).max() < 1e-9
    # a problem with a frame that nobody observes and an empty problem are handled, not crashed on
    empty = aar.Dataset.__new__(aar.Dataset)
    empty.__dict__.update(ds.__dict__)
    for k in ("obs_frame", "obs_cam", "obs_marker"):
        setattr(empty, k, np.zeros(0, dtype=np.int32))
    empty.obs_uv = np.zeros((0, 8), dtype=np.float32)
    empty.num_obs = 0
    with Problem(empty) as p:
        r, ss = p.eval_residuals(empty.x_full)
        assert len(r) == 0 and ss == 0.0


def test_full_size_config3_properties():
    # BASELINE.json configs[2] (8 cameras / 40 markers / 500 frames): size-independent properties
    ds = aar.synth(3)
    with Problem(ds) as p:
        x, rep = p.lm_solve(ds.x_full)
        err = [t["err"] for t in rep["trace"]]
        assert all(b < a for a, b in zip([rep["initial_err"]] + err[:-1], err))     # monotone decrease
        mu = [t["mu"] for t in rep["trace"]]
        np.testing.assert_allclose(np.array(mu[1:]) / np.array(mu[:-1]), 0.33, rtol=1e-12)
        rmse, ss = p.reproj_stats(x)
        assert abs(rmse - 0.3 * np.sqrt(2)) < 0.02                                  # the noise floor
        # idempotence: restarting from the solution stops after one step
        x2, rep2 = p.lm_solve(x)
        assert rep2["iterations"] == 1 and abs(rep2["final_err"] - rep["final_err"]) < 1e-4 * 8 * ds.num_obs
        # sum of squares is the checksum of the residual rows
        r, ss2 = p.eval_residuals(x)
        np.testing.assert_allclose(ss2, float((r ** 2).sum()), rtol=1e-12)
        # the gradient vanishes at the optimum relative to where it started
        _, B0, _ = p.eval_normal_equations(ds.x_full)
        _, B1, _ = p.eval_normal_equations(x)
        assert np.abs(B1).max() < 1e-3 * np.abs(B0).max()


def test_config4_size_against_oracle():
    # BASELINE.json configs[3] (8 cameras / 40 markers / 2000 frames, 50 k marker observations) at full size: residual rows
    # bit-exact, one damped step against the oracle's sparse LDL^T (12 276 unknowns), three reduced-system tiles
    ds = aar.synth(4)
    o = ol.Oracle(ds)
    with Problem(ds) as p:
        r, ss = p.eval_residuals(ds.x_full)
        assert np.array_equal(r, o.residuals(ds.x_full, res_mode=ol.RES_F32))
        mu = 1e6
        d = p.eval_damped_step(ds.x_full, mu)
        do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        assert np.abs(d - do).max() / np.abs(do).max() < 1e-9
        x, rep = p.lm_solve(ds.x_full)
        rmse, _ = p.reproj_stats(x)
        assert rep["iterations"] < 30 and abs(rmse - 0.3 * np.sqrt(2)) < 0.02


def test_full_size_config5_properties():
    # BASELINE.json configs[4] (16 cameras / 200 markers / 5000 frames, 1.26 M marker observations = 10 M residual rows), the
    # largest size: the oracle's sparse LDL^T needs minutes and > 15 GB per step here, so parity goes through properties
    ds = aar.synth(5)
    assert ds.num_obs > 1_200_000
    o = ol.Oracle(ds)
    with Problem(ds) as p:
        # residual rows bit-exact against the oracle (a pure streaming pass on the CPU)
        r, ss = p.eval_residuals(ds.x_full)
        ro = o.residuals(ds.x_full, res_mode=ol.RES_F32)
        assert np.array_equal(r, ro)
        np.testing.assert_allclose(ss, float((ro.astype(np.float64) ** 2).sum()), rtol=1e-12)
        # a damped step from the start is a descent step
        d = p.eval_damped_step(ds.x_full, 1e3)
        assert p.eval_residuals(ds.x_full + d, want_vector=False)[1] < ss
        x, rep = p.lm_solve(ds.x_full)
        rmse, _ = p.reproj_stats(x)
        err = [t["err"] for t in rep["trace"]]
        assert all(b < a for a, b in zip([rep["initial_err"]] + err[:-1], err))
        assert rep["iterations"] < 40 and abs(rmse - 0.3 * np.sqrt(2)) < 0.01
        # idempotence at the optimum
        x2, rep2 = p.lm_solve(x)
        assert rep2["iterations"] == 1
        # cameras come out at the ground truth (gauge fixed by the root camera / marker)
        np.testing.assert_allclose(x[:6 * (ds.num_cams - 1)], ds.x_truth[:6 * (ds.num_cams - 1)], atol=2e-3)

    # the same solve sharded over four ranks (frame ranges, one all-reduce of S | rhs | g0 per try): identical trace
    def run(comm, rank):
        with Problem(ds, comm=comm) as q:
            xs, reps = q.lm_solve(ds.x_full)
            return xs, reps, q.local_obs
    out = _run_ranks(4, run)
    assert sum(o_[2] for o_ in out) == ds.num_obs
    for xs, reps, _ in out:
        np.testing.assert_allclose([t["err"] for t in reps["trace"]], err, rtol=1e-9)
        np.testing.assert_allclose(xs, x, atol=1e-8)


@pytest.mark.parametrize("name,split", [("g1_cfg2", "1"), ("g1_cfg3_cut", "3")])
def test_schur_mfma_kernel_forced_on_small_problems(name, split, monkeypatch):
    # the block-of-S-stationary MFMA Schur kernel (normally A >= 96) forced on the golden problems: odd frame ranges, a
    # partial last entity group, blocks of S on and off the diagonal; same damped step and LM trace as the oracle / golden
    ds, g = load_golden(name)
    o = ol.Oracle(ds)
    monkeypatch.setenv("AAR_SCHUR_MFMA", "1")
    monkeypatch.setenv("AAR_SCHUR_SPLIT", split)
    with Problem(ds, residual_mode=aar.RES_F64) as p:
        Ho, _ = o.normal_equations(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
        for mu in (float(np.diag(Ho).max()) * 1e-3, 1.0):
            d = p.eval_damped_step(ds.x_full, mu)
            do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-8, mu
    with Problem(ds) as p:
        x, rep = p.lm_solve(ds.x_full)
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], g["analytic_err"], rtol=1e-7)
        np.testing.assert_allclose(x, g["analytic_x"], atol=1e-7)


@pytest.mark.parametrize("mfma,cams,markers,frames", [("0", 4, 62, 40), ("1", 4, 62, 40), ("0", 4, 20, 60), ("0", 3, 29, 50)])
def test_tile_counts_and_schur_kernels_against_oracle(mfma, cams, markers, frames, monkeypatch):
    # 4 cameras / 62 markers / 40 frames: A = 66 shared entities (5 entity groups of 16, a partial last one), 5 tiles of the
    # reduced system, both Schur kernels; 4 / 20 / 60: exactly two tiles (A = 24, n = 144); 3 / 29 / 50: two full tiles (n = 192)
    monkeypatch.setenv("AAR_SCHUR_MFMA", mfma)
    ds = aar.synth(3, num_cams=cams, num_markers=markers, num_frames=frames)
    o = ol.Oracle(ds)
    with Problem(ds) as p:
        r, ss = p.eval_residuals(ds.x_full)
        assert np.array_equal(r, o.residuals(ds.x_full, res_mode=ol.RES_F32))
        for mu in (1e6, 1e2):
            d = p.eval_damped_step(ds.x_full, mu)
            do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-8, mu
        x, rep = p.lm_solve(ds.x_full)
        rmse, _ = p.reproj_stats(x)
        assert rep["iterations"] < 40 and abs(rmse - 0.3 * np.sqrt(2)) < 0.05   # (few observations per unknown: the fit absorbs some noise)


@pytest.mark.parametrize("opt", [(True, True, True), (False, True, True), (True, False, True)])
def test_gauge_rows_in_trailing_tiles_of_a_three_tile_system(opt):
    # 18 cameras / 20 markers: the root marker's rows (entity 18 -> rows 108..113) and, with a group switched off, whole runs of
    # fixed entities fall in the SECOND and THIRD tile of a three-tile system, i.e. they get their damping / identity rows on
    # first touch inside the fused panel kernel (slabs, output blocks, right-hand side) instead of the diagonal-tile kernel
    ds = aar.synth(3, num_cams=18, num_markers=20, num_frames=40)
    o = ol.Oracle(ds, optimize=opt)
    with Problem(ds, optimize=opt) as p:
        assert p.num_vars == o.num_vars
        for mu in (1e5, 10.0):
            d = p.eval_damped_step(ds.x_full, mu)
            do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-8, mu
        x, rep = p.lm_solve(ds.x_full)
        assert rep["iterations"] < 40 and rep["final_err"] < rep["initial_err"]


@pytest.mark.parametrize("env", [{"AAR_FUSED_PANEL": "0"}, {"AAR_BS_RIDES": "0"}, {"AAR_FUSED_PANEL": "0", "AAR_BS_RIDES": "0"}, {"AAR_FUSED_PANEL": "5"}, {"AAR_FUSED_PANEL": "2"},
                                 {"AAR_DENSE_FROM_PASSA": "0", "AAR_SCHUR_MFMA": "1"}, {"AAR_LDL_LOOKAHEAD": "0"},
                                 {"AAR_LDL_LOOKAHEAD": "0", "AAR_FUSED_PANEL": "0"}, {"AAR_INIT_HEADSTART": "0"}])
def test_dense_solve_path_switches(env):
    # The dense LDL^T has alternative launch structures behind environment switches that libaar reads ONCE per process (the
    # two-kernel panel solve + trailing update instead of the fused k_ldl_panel, the chained k_ldl_backsolve instead of the
    # back-substitution riding in the last tile's launch, the fused panel kernel on taller block columns): a fresh interpreter
    # per combination solves systems of 2, 3 and 5 tiles against the oracle's Eigen-checked LDL^T.
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import aar, oracle_lib as ol
        worst = 0.0
        for cams, markers, frames in ((4, 20, 60), (8, 40, 60), (4, 62, 40)):
            ds = aar.synth(3, num_cams=cams, num_markers=markers, num_frames=frames)
            o = ol.Oracle(ds)
            with aar.Problem(ds, solver="direct") as p:
                for mu in (1e6, 1e2):
                    d = p.eval_damped_step(ds.x_full, mu)
                    do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
                    worst = max(worst, float(np.abs(d - do).max() / np.abs(do).max()))
                x, rep = p.lm_solve(ds.x_full)
                assert rep["iterations"] < 40, rep["iterations"]
        print("WORST", worst)
    """) % (os.path.join(os.path.dirname(__file__), "..", "automatic-ar_amd"), os.path.dirname(__file__))
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    worst = float([l for l in out.stdout.splitlines() if l.startswith("WORST")][-1].split()[1])
    assert worst < 1e-8, (env, worst)


@pytest.mark.parametrize("lookahead", ["1", "0"])
def test_dense_lookahead_seven_tiles(lookahead):
    # Tall block columns (more than three tiles below the diagonal) take k_ldl_trsm and then NO update launch: the next diagonal tile's
    # workgroup applies the column's update to its own tile (first touch included, for column 0) while riders of that launch do the other
    # tiles and the right-hand side.  A seven-tile system (four such columns, then the fused panels) against the oracle's LDL^T, both ways.
    # Sixteen cameras put the root marker -- a gauge entity: identity rows, zero right-hand side -- at the FIRST row of tile 1, whose first touch
    # (damping, gauge) then happens in that tile's look-ahead prologue.
    import subprocess, sys, textwrap
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import aar, oracle_lib as ol
        ds = aar.synth(3, num_cams=16, num_markers=92, num_frames=120)
        o = ol.Oracle(ds)
        worst = 0.0
        with aar.Problem(ds, solver="direct") as p:
            for mu in (1e4, 1e-2):
                d = p.eval_damped_step(ds.x_full, mu)
                do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
                worst = max(worst, float(np.abs(d - do).max() / np.abs(do).max()))
            x, rep = p.lm_solve(ds.x_full)
            assert rep["iterations"] < 40 and rep["final_err"] < rep["initial_err"]
        print("WORST", worst, "N", ds.num_vars)
    """) % (os.path.join(os.path.dirname(__file__), "..", "automatic-ar_amd"), os.path.dirname(__file__))
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, "AAR_LDL_LOOKAHEAD": lookahead}, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    worst = float([l for l in out.stdout.splitlines() if l.startswith("WORST")][-1].split()[1])
    assert worst < 1e-8, (lookahead, worst)


def test_randomized_shapes_against_oracle():
    # a sweep over sizes that move every structural parameter at once: camera / marker counts (shared system n from 18 to ~400,
    # i.e. one to five 96-wide tiles, n not a multiple of 16 or 96), frames from a handful to a few hundred (ragged visibility),
    # every optimise-flag combination now and then, sharded over 2-3 ranks for every third shape
    rng = np.random.default_rng(20190219)
    done = 0
    for k in range(40):
        C, M, F = int(rng.integers(3, 11)), int(rng.integers(4, 60)), int(rng.integers(2, 160))
        try:
            ds = aar.synth(3, num_cams=C, num_markers=M, num_frames=F, seed=int(rng.integers(1, 2 ** 31)))
        except aar.AarError:
            continue                      # no frame with two observations at this size
        if ds.num_obs < 20:
            continue
        opt = [(True, True, True), (True, True, True), (False, True, True), (True, False, True)][k % 4]
        o = ol.Oracle(ds, optimize=opt)
        with Problem(ds, optimize=opt) as p:
            r, ss = p.eval_residuals(ds.x_full)
            assert np.array_equal(r, o.residuals(ds.x_full, res_mode=ol.RES_F32)), (C, M, F)
            mu = float(10.0 ** rng.integers(0, 7))
            d = p.eval_damped_step(ds.x_full, mu)
            do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-7, (C, M, F, mu)
            x, rep = p.lm_solve(ds.x_full)
        xo, repo = o.lm_solve(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        assert abs(rep["iterations"] - repo["iterations"]) <= 1, (C, M, F)
        np.testing.assert_allclose(rep["final_err"], repo["final_err"], rtol=1e-5, err_msg=str((C, M, F)))
        if k % 3 == 0 and opt == (True, True, True):
            def solve(comm, rank, ds=ds):
                with Problem(ds, comm=comm) as q:
                    return q.lm_solve(ds.x_full)
            for xs, reps in _run_ranks(2 + k % 2, solve):
                assert reps["iterations"] == rep["iterations"], (C, M, F)
                np.testing.assert_allclose(reps["final_err"], rep["final_err"], rtol=1e-8)
        done += 1
        if done >= 9:
            break
    assert done >= 7


def test_single_rank_communicator_path():
    # world_size 1 through RCCL: exercises the sharded code path (all-reduces of S, rhs, scalars) on one GPU
    ds, g = load_golden("g1_cfg2")
    comm = aar.Comm(aar.Comm.make_id(), 1, 0, 0)
    try:
        with Problem(ds, comm=comm) as p:
            x, rep = p.lm_solve(ds.x_full)
            np.testing.assert_allclose([t["err"] for t in rep["trace"]], g["analytic_err"], rtol=1e-7)
            np.testing.assert_allclose(x, g["analytic_x"], atol=1e-7)
    finally:
        comm.close()


@pytest.mark.gpu
def test_remove_distortions_kernel_equals_oracle():
    # MultiCamMapper::remove_distortions (libs/multicam_mapper.cpp:554-578): the undistortPoints kernel against the oracle's
    # restatement, float outputs bit for bit; 5-, 8- and 12-coefficient vectors, none, a non-zero skew, in-place call
    rng = np.random.default_rng(11)
    K = np.array([[1432.1, 0.3, 961.0], [0, 1429.8, 539.5], [0, 0, 1]])
    uv = np.stack([rng.uniform(0, 1920, 100003), rng.uniform(0, 1080, 100003)], axis=1).astype(np.float32)
    for dist in ([-0.11, 0.085, 0.0012, -0.0007, -0.019], [0.2, -0.1, 0.001, 0.002, 0.01, 0.3, -0.05, 0.004],
                 [0.05, 0.01, 0.001, 0.0, 0.002, 0.01, 0.0, 0.0, 1e-3, -2e-4, 5e-4, 1e-4], []):
        got = aar.undistort_points(K, dist, uv)
        ref = ol.undistort_points(K, dist, uv)
        assert np.array_equal(got, ref), dist
    assert aar.undistort_points(K, [0.1], uv[:0]).shape == (0, 2)


def _run_rank(group, rank, ds, out, with_huber=False):
    comm = aar.Comm.local(group, rank, 0)
    try:
        with Problem(ds, comm=comm, with_huber=with_huber) as p:
            x, rep = p.lm_solve(ds.x_full)
            out[rank] = (x, rep, p.local_obs)
    except Exception as e:   # a rank that dies would leave the others waiting at a barrier: report, do not hang the test
        out[rank] = e
    finally:
        comm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world,name", [(2, "g1_cfg2"), (3, "g1_cfg2"), (8, "g1_cfg2"), (4, "g1_cfg3_cut")])
def test_sharded_lm_on_one_gpu_through_the_local_group(world, name):
    # The multi-rank path -- frame-range shards, all-reduces of S | rhs, of the step's scalars and of the initial diagonal,
    # the final gather -- with `world` ranks as host threads on ONE GPU (the in-process transport replaces RCCL, nothing else
    # changes): every rank must return the single-GPU trace and the full pose vector
    import threading
    ds, g = load_golden(name)
    group = aar.LocalGroup(world)
    out = [None] * world
    th = [threading.Thread(target=_run_rank, args=(group, r, ds, out), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    group.close()
    for r in range(world):
        assert not isinstance(out[r], Exception), out[r]
        x, rep, nloc = out[r]
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], g["analytic_err"], rtol=1e-7)
        np.testing.assert_allclose(x, g["analytic_x"], atol=1e-7)
    assert sum(o[2] for o in out) == ds.num_obs
    assert all(np.array_equal(out[0][0], o[0]) for o in out[1:])   # fixed reduction order: identical bits on every rank


def _run_ranks(world, fn):
    import threading
    group = aar.LocalGroup(world)
    out = [None] * world

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            out[r] = fn(comm, r)
        except Exception as e:
            out[r] = e
        finally:
            comm.close()
    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    group.close()
    for o in out:
        assert not isinstance(o, Exception), o
    return out


@pytest.mark.gpu
def test_sharded_huber_schedule_and_idle_rank():
    # (1) -with-huber on 4 ranks: the weights and optCallBack's delta schedule give the single-GPU result;
    # (2) more ranks than frames: a rank that owns no frame still takes part in every collective
    ds, g = load_golden("g1_cfg2_huber")
    with Problem(ds, with_huber=True) as p:
        x1, rep1 = p.lm_solve(ds.x_full)

    def solve_h(comm, r):
        with Problem(ds, comm=comm, with_huber=True) as p:
            return p.lm_solve(ds.x_full)
    for x, rep in _run_ranks(4, solve_h):
        assert rep["iterations"] == rep1["iterations"]
        # (a 505-step run: the per-rank sums are taken in another order, the trajectories drift by ~2e-7 relative)
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], [t["err"] for t in rep1["trace"]], rtol=1e-5)
        np.testing.assert_allclose(x, x1, atol=1e-5)

    small = aar.synth(2, num_cams=3, num_markers=8, num_frames=2)
    with Problem(small) as p:
        xs, reps = p.lm_solve(small.x_full)

    def solve_s(comm, r):
        with Problem(small, comm=comm) as p:
            return p.lm_solve(small.x_full) + (p.local_obs,)
    outs = _run_ranks(3, solve_s)
    assert sorted(o[2] for o in outs)[0] == 0            # one rank has nothing
    for x, rep, _ in outs:
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], [t["err"] for t in reps["trace"]], rtol=1e-8)
        np.testing.assert_allclose(x, xs, atol=1e-8)


def test_sharded_retry_and_mispredicted_damping():
    # (1) far start + tau = 1e-6 (golden retry fixture): rejected tries, the blocks of the current point are rebuilt;
    # (2) the -with-huber fixture: late in its 505 steps an accepted step has a gain far below 0.94, so its damping is NOT the
    #     predicted 0.33 mu -- on the multi-GPU path the speculative system of such a step has already been all-reduced together
    #     with the step's scalars, so the rank's shared blocks are rebuilt from its observations (pass B alone) before the new
    #     Schur complement.
    # Three ranks must reproduce the single-GPU trace, try for try, with the fused collective and without it.
    ds_r, g = load_golden("g1_cfg2_retry")
    ds_h, gh = load_golden("g1_cfg2_huber")
    for ds, prm_kw, hub in ((ds_r, dict(tau=float(g["tau"][0])), False), (ds_h, dict(), True)):
        with Problem(ds, with_huber=hub) as p:
            x1, rep1 = p.lm_solve(ds.x_full, params=aar.lm_default_params(**prm_kw), trace_cap=600)
        tries1 = np.array([t["tries"] for t in rep1["trace"]])
        mu1 = np.array([t["mu"] for t in rep1["trace"]])
        err1 = np.array([t["err"] for t in rep1["trace"]])
        if hub:
            odd = np.nonzero((tries1[1:] == 1) & (np.abs(mu1[1:] / mu1[:-1] - 0.33) > 1e-6))[0]
            assert len(odd) >= 1                                        # an accepted step with another damping than predicted
            k = int(odd[0]) + 3
        else:
            assert tries1.max() > 1                                     # a rejected try
            k = 6

        def solve(comm, r):
            with Problem(ds, comm=comm, with_huber=hub) as q:
                return q.lm_solve(ds.x_full, params=aar.lm_default_params(**prm_kw), trace_cap=600)
        for fused in ("1", "0"):
            os.environ["AAR_FUSED_COMM"] = fused
            try:
                outs = _run_ranks(3, solve)
            finally:
                del os.environ["AAR_FUSED_COMM"]
            for x, rep in outs:
                k = min(k, len(rep["trace"]), len(tries1))
                assert [t["tries"] for t in rep["trace"]][:k] == tries1[:k].tolist()
                np.testing.assert_allclose([t["err"] for t in rep["trace"]][:k], err1[:k], rtol=1e-5)
                np.testing.assert_allclose([t["mu"] for t in rep["trace"]][:k], mu1[:k], rtol=1e-3)
                assert abs(np.sqrt(rep["final_err"] / (4 * ds.num_obs)) - np.sqrt(rep1["final_err"] / (4 * ds.num_obs))) < 1e-4


def test_config1_box_like_find_solution_vs_compiled_reference(tmp_path):
    # BASELINE.json configs[0] (box data set: 3 cameras / ~6 markers, marker_size 0.05; the data set itself is not in the
    # container, README.md:55-56 -- `--synth 1` writes a stand-in in the reference's file formats).  The whole find_solution
    # flow (apps/find_solution.cpp:101-163) on the HIP path -- calib folders + aruco.detections -> Initializer -> initial.solution
    # -> LM -> final.solution -- against the REAL reference solver (oracle/_ref: libs/sparselevmarq.h + Eigen compiled in place)
    # started from the very same initial.solution with the reference-faithful residual / central-difference float Jacobian.
    import subprocess
    from conftest import PKG
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "box")
    assert subprocess.run([exe, "--synth", "1", folder], capture_output=True, text=True).returncode == 0
    os.remove(os.path.join(folder, "initial.solution"))           # the driver must write its own from the Initializer
    run = subprocess.run([exe, folder, "0.05"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    assert "Initializer:" in run.stdout and "The algorithm took:" in run.stdout
    init = aar.solution_read(os.path.join(folder, "initial.solution"))
    fin = aar.solution_read(os.path.join(folder, "final.solution"))
    assert init.num_cams == 3 and 5 <= init.num_markers <= 6 and init.num_frames > 100   # (the box's bottom face is never seen)
    assert fin.num_obs == init.num_obs and np.array_equal(fin.obs_uv, init.obs_uv)
    o = ol.Oracle(init)
    solve = o.ref_lm_solve if ol.have_ref() else o.lm_solve
    x_ref, rep_ref = solve(init.x_full, jac_mode=ol.JAC_NUMERIC_F32, res_mode=ol.RES_F32)
    rmse_ref = o.reproj_stats(x_ref)["rmse"]
    rmse_gpu = o.reproj_stats(fin.x_full)["rmse"]
    rmse_init = o.reproj_stats(init.x_full)["rmse"]
    assert rmse_gpu < rmse_init
    assert abs(rmse_gpu - rmse_ref) < 1e-4, (rmse_gpu, rmse_ref)        # the north star's bar
    # the same solve through the C ABI from the file: same iteration count as the driver printed, same final error
    with Problem(init) as p:
        x, rep = p.lm_solve(init.x_full)
        assert ("LM iterations: %d " % rep["iterations"]) in run.stdout
        assert abs(p.reproj_stats(x)[0] - rmse_gpu) < 1e-7               # final.solution stores vec -> mat -> vec
        assert abs(rep["iterations"] - rep_ref["iterations"]) <= 2


def test_full_size_config3_against_compiled_reference():
    # BASELINE.json's metric configuration (8 cameras / 40 markers / 500 frames) at FULL size against the real reference solver
    # (oracle/_ref) on the same detections: one damped step against the oracle's sparse LDL^T of the same analytic system, and
    # the complete solve: final sum of squares / RMSE of the reference-faithful CPU run (numeric float Jacobian) within the
    # north star's 1e-4 px.  (~10 s of CPU for the reference solve.)
    ds = aar.synth(3)
    o = ol.Oracle(ds)
    solve = o.ref_lm_solve if ol.have_ref() else o.lm_solve
    x_ref, rep_ref = solve(ds.x_full, jac_mode=ol.JAC_NUMERIC_F32, res_mode=ol.RES_F32, threads=min(32, os.cpu_count() or 1))
    with Problem(ds) as p:
        mu = 1e5
        d = p.eval_damped_step(ds.x_full, mu)
        do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        assert np.abs(d - do).max() / np.abs(do).max() < 1e-9
        x, rep = p.lm_solve(ds.x_full)
        rmse, ss = p.reproj_stats(x)
    st = o.reproj_stats(x_ref)
    assert abs(rmse - st["rmse"]) < 1e-4, (rmse, st["rmse"])
    assert abs(rmse - st["rmse"]) < 1e-6                                   # what is observed: 5e-8 px
    np.testing.assert_allclose(rep["final_err"], rep_ref["final_err"], rtol=1e-5)   # 8873.4574 vs 8873.4597 in round 1
    assert abs(rep["iterations"] - rep_ref["iterations"]) <= 1
    assert np.abs(x - x_ref).max() < 1e-3


def test_solver_seam_step_callback_and_stop_function():
    # ucoslam::SparseLevMarq<T>::setStepCallBackFunc / setStopFunction (libs/sparselevmarq.h:121-123) through the C ABI: the step
    # callback sees curr_z after every step (:463); with a stop function the loop is do { step; callback } while (!stop) (:444-450)
    ds, g = load_golden("g1_cfg2")
    with Problem(ds) as p:
        seen = []
        p.set_step_callback(lambda z: seen.append(z))
        x, rep = p.lm_solve(ds.x_full)
        assert len(seen) == rep["iterations"] == int(g["analytic_iterations"][0])
        assert np.array_equal(seen[-1], p.extract_z(x))                       # the last curr_z is the returned solution
        assert all(len(z) == p.num_vars for z in seen) and not np.array_equal(seen[0], seen[1])
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], g["analytic_err"], rtol=1e-7)
        # a stop function that halts after k steps reproduces the first k entries of the golden trace
        k, calls = 5, []
        p.set_stop_function(lambda z: calls.append(z) or len(calls) >= k)
        x2, rep2 = p.lm_solve(ds.x_full, params=aar.lm_default_params(max_iters=2))   # max_iters is ignored on this branch (:444)
        assert rep2["iterations"] == k and len(calls) == k
        np.testing.assert_allclose([t["err"] for t in rep2["trace"]], g["analytic_err"][:k], rtol=1e-7)
        np.testing.assert_allclose(p.extract_z(x2), seen[k - 1], rtol=0, atol=1e-12)
        assert len(seen) == rep["iterations"] + k                                # the step callback ran on this branch too (:449)
        p.set_stop_function(None)
        p.set_step_callback(None)
        x3, rep3 = p.lm_solve(ds.x_full, params=aar.lm_default_params())   # (NULL params would keep the max_iters = 2 set above)
        assert rep3["iterations"] == rep["iterations"] and len(seen) == rep["iterations"] + k


def test_huber_schedule_through_the_step_callback():
    # MultiCamMapper::solve installs optCallBack as the solver's step callback and sets hubberDelta = 10 itself
    # (libs/multicam_mapper.cpp:412-425); a caller doing the same through the seam gets the built-in schedule's trace
    ds, g = load_golden("g1_cfg2_huber")
    with Problem(ds, with_huber=True) as p:
        delta = [np.float32(10.0)]

        def opt_callback(z):
            assert z is None                                   # want_z = False: no device -> host copy per step
            if delta[0] > 2.5:
                delta[0] = np.float32(np.float64(delta[0]) - 7.5 / 500)       # float -= double
            p.set_huber_delta(float(delta[0]))
        p.set_step_callback(opt_callback, want_z=False)
        p.set_huber_delta(10.0)
        x, rep = p.lm_solve(ds.x_full, trace_cap=600)
        assert rep["iterations"] == int(g["analytic_iterations"][0])
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], g["analytic_err"], rtol=1e-5)
        assert abs(p.get_huber_delta() - 2.5) < 0.02


def test_cpp_mirror_constructor_init_and_solver_seam(tmp_path):
    # the C++ classes a maintainer would swap in for the reference's (automatic-ar_amd/host/multicam_mapper.h): the 8-argument
    # MultiCamMapper constructor (libs/multicam_mapper.h:17) must reach the same solution as the mapper built from the data set,
    # init(object_poses, fcm) + track() (apps/track.cpp:127-131) and SparseLevMarq's callbacks work through the mirror
    import subprocess
    from conftest import PKG, ROOT
    exe = str(tmp_path / "mapper_api_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "mapper_api_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, "2"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = dict(l.split(" = ") for l in run.stdout.splitlines() if " = " in l)
    ds = aar.synth(2)
    assert "the very initial error:" in run.stdout                                   # libs/multicam_mapper.cpp:333
    assert int(kv["ctor_num_vars"]) == ds.full_len + 9 * ds.num_cams                  # default Config: intrinsics counted (:239-250)
    assert int(kv["ctor_iterations"]) == int(kv["direct_iterations"])
    # (transforms went through 4x4 matrices and back, and the corners through remove_distortions' undistort / re-project with
    #  zero distortion, which moves some float corners by an ulp: the two solves agree to that, not to the last bit)
    np.testing.assert_allclose(float(kv["ctor_final_err"]), float(kv["direct_final_err"]), rtol=1e-5)
    assert float(kv["ctor_vs_direct_max_abs"]) < 1e-5
    assert int(kv["seam_steps"]) == 4 and int(kv["seam_callbacks"]) == 4 and int(kv["seam_zlen"]) == ds.full_len
    assert float(kv["seam_final_err"]) <= float(kv["direct_final_err"]) * (1 + 1e-9)
    assert int(kv["track_frames"]) == ds.num_frames and float(kv["track_max_err"]) < 100.0
    # the default Config (intrinsics on) through the mirror: fx and cy come back from a calibration set 1 % / 2 px off
    assert int(kv["intr_num_vars"]) == int(kv["intr_io_vec"]) == ds.full_len + 9 * ds.num_cams
    assert float(kv["intr_final_err"]) < float(kv["intr_initial_err"]) and float(kv["intr_final_err"]) < 1.05 * float(kv["direct_final_err"])
    assert abs(float(kv["intr_fx0"]) - 1000.0) < 6.0 and abs(float(kv["intr_cy0"]) - 360.0) < 3.0    # (weakly determined by 390 observations: fx 1010 -> 1003.8, cy 358 -> 361.7)
    np.testing.assert_allclose(float(kv["intr_err_fn"]), float(kv["intr_final_err"]), rtol=1e-12)   # error_function(io_vec) at the solution


def test_unsupported_sizes_are_refused_collectively():
    # the two LDS-resident structures bound what a problem may look like: a frame that touches more than
    # ~800 cameras+markers (pass A in wrench form keeps 25 doubles per frame-local slot in LDS: the guard is sized by the form that is launched; the row
    # form of rounds 1-3 stopped at ~300), more than ~560 cameras+markers in all ON THE OUTPUT-STATIONARY KERNEL -> AAR_ERR_UNSUPPORTED, never a wrong answer; on a sharded
    # problem EVERY rank gets the status, also the ranks whose own frames are fine (nobody is left waiting in a collective)
    def dataset(num_markers, wide_frame):
        ds = aar.Dataset()
        ds.num_cams, ds.num_markers, ds.num_frames, ds.root_cam, ds.root_marker = 2, num_markers, 4, 0, 0
        ds.marker_size = 0.05
        ds.cam_ids = np.arange(2, dtype=np.int32); ds.marker_ids = np.arange(num_markers, dtype=np.int32)
        ds.frame_ids = np.arange(4, dtype=np.int32)
        ds.image_sizes = np.tile(np.array([1280, 720], dtype=np.int32), (2, 1))
        ds.cam_mats = np.tile(np.array([1000.0, 0, 640, 0, 1000, 360, 0, 0, 1]), (2, 1))
        ds.dist_coeffs = np.zeros((2, 5))
        f, c, m = [], [], []
        for fr in range(4):
            mk = np.arange(wide_frame if fr == 3 else 3)      # the LAST frame sees `wide_frame` markers
            f += [fr] * len(mk); c += [0] * len(mk); m += list(mk)
        ds.obs_frame, ds.obs_cam, ds.obs_marker = (np.array(v, dtype=np.int32) for v in (f, c, m))
        ds.num_obs = len(f)
        ds.obs_uv = np.tile(np.array([600, 300, 650, 300, 650, 350, 600, 350], dtype=np.float32), (ds.num_obs, 1))
        ds.x_full = np.zeros(6 * (2 - 1) + 6 * (num_markers - 1) + 6 * 4)
        ds.x_full[2::6] = 0.0
        ds.x_truth = None
        ds.optimize_cam_poses = ds.optimize_marker_poses = ds.optimize_object_poses = True
        ds.optimize_cam_intrinsics = False
        return ds
    with pytest.raises(aar.AarError) as e:
        Problem(dataset(1100, 1000))
    assert e.value.code == aar.AAR_ERR_UNSUPPORTED and "touches" in str(e.value)
    Problem(dataset(400, 340)).close()                 # (refused until round 4, when the guard still priced the row form: 340 slots are 68 KB in wrench form)
    os.environ["AAR_PASSA_WRENCH"] = "0"
    try:
        with pytest.raises(aar.AarError) as e:
            Problem(dataset(400, 340))                 # ... and still refused when the row form is what would be launched
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED and "touches" in str(e.value)
    finally:
        del os.environ["AAR_PASSA_WRENCH"]
    # > ~560 cameras+markers: only the OUTPUT-STATIONARY Schur kernel keeps a row panel of all of them in LDS; the MFMA kernel
    # (the default from 96 entities) has no such panel, so the problem is fine unless that kernel is ruled out -- switched off,
    # or its dense panels over the memory budget
    Problem(dataset(700, 3)).close()
    for knob, val in (("AAR_SCHUR_MFMA", "0"), ("AAR_SCHUR_PANEL_MB", "0")):
        os.environ[knob] = val
        try:
            with pytest.raises(aar.AarError) as e:
                Problem(dataset(700, 3))
            assert e.value.code == aar.AAR_ERR_UNSUPPORTED and "exceed" in str(e.value)
        finally:
            del os.environ[knob]
    Problem(dataset(400, 280)).close()                 # inside both limits

    wide = dataset(1100, 1000)
    def create(comm, rank):
        try:
            Problem(wide, comm=comm).close()
            return "created"
        except aar.AarError as err:
            return err.code
    out = _run_ranks(2, create)                            # frames 0-1 / 2-3 by observation count: only the last rank holds the wide frame
    assert out == [aar.AAR_ERR_UNSUPPORTED, aar.AAR_ERR_UNSUPPORTED]


def test_intrinsics_block_against_oracle_and_real_solver():
    # MultiCamMapper::Config::optimize_cam_intrinsics (the reference's default Config; libs/multicam_mapper.cpp:488-498,580-593,
    # 788-798,835-893): 9 more entries per camera at the end of every vector.  Rows bit-exact, J^T J / B of the analytic columns,
    # damped step, the LM trace of the real solver driven with the same Jacobian; the distortion entries never move
    ds, g = load_golden("g1_cfg2_intr")
    o = ol.Oracle(ds, intrinsics=True)
    i0 = ds.full_len
    with Problem(ds, intrinsics=True) as p:
        assert p.full_len == ds.full_len + 9 * ds.num_cams and p.num_vars == o.num_vars
        x0 = p.x_with_intrinsics(ds.x_full)
        np.testing.assert_array_equal(p.extract_z(x0), o.extract_z(ds.x_full))
        r, ss = p.eval_residuals(x0)
        assert np.array_equal(r, g["r0_f32"])
        H, B, _ = p.eval_normal_equations(x0)
        Ho, Bo = o.normal_equations(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        assert np.abs(H - Ho).max() / np.abs(Ho).max() < 1e-12
        assert np.abs(B - Bo).max() / np.abs(Bo).max() < 1e-11
        assert not H[i0:, :].reshape(-1, 9, H.shape[1])[:, 4:, :].any()            # distortion rows / columns: exact zeros
        for mu in (float(np.diag(Ho).max()), 1e3):
            d = p.eval_damped_step(x0, mu)
            do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-8, mu
            assert not d[i0:].reshape(-1, 9)[:, 4:].any()
        x, rep = p.lm_solve(x0)
        assert rep["iterations"] == int(g["analytic_iterations"][0])
        np.testing.assert_allclose([t["err"] for t in rep["trace"]], g["analytic_err"], rtol=1e-7)
        np.testing.assert_allclose(p.extract_z(x), g["analytic_z"], atol=1e-6)
        np.testing.assert_array_equal(x[i0:].reshape(-1, 9)[:, 4:], ds.dist_coeffs)
        assert np.abs(x[i0:].reshape(-1, 9)[:, :4] - x0[i0:].reshape(-1, 9)[:, :4]).max() > 0.5      # the intrinsics did move
        # reprojection error at the solved intrinsics: below the reference-faithful run's (see tests/test_oracle_golden.py)
        rmse = np.sqrt(float((o.residuals(ds.x_full, p.extract_z(x), res_mode=ol.RES_F64) ** 2).sum()) / (4 * ds.num_obs))
        assert abs(rmse - g["analytic_rmse"][0]) < 1e-7 and rmse <= g["faithful_rmse"][0] + 1e-9
        assert abs(rmse - g["faithful_rmse"][0]) < 1e-3

    def solve(comm, rank):
        with Problem(ds, intrinsics=True, comm=comm) as q:
            return q.lm_solve(q.x_with_intrinsics(ds.x_full))
    for xs, reps in _run_ranks(3, solve):                                           # sharded: intrinsics entities are shared ones
        np.testing.assert_allclose([t["err"] for t in reps["trace"]], [t["err"] for t in rep["trace"]], rtol=1e-8)
        np.testing.assert_allclose(xs, x, atol=1e-7)
    # a fixed-intrinsics problem on the same data keeps the calibration's skew: other rows, other optimum
    with Problem(ds) as p:
        assert not np.array_equal(p.eval_residuals(ds.x_full)[0], g["r0_f32"])


def test_huber_schedule_with_a_rejected_try():
    # -with-huber from a far start with a tiny tau: step 22 needs three damping tries.  After a rejected try the blocks of the
    # current point are rebuilt; B = -J^T x64 must then carry the residual weights of the Huber delta that was in force when the
    # point was ACCEPTED (libs/sparselevmarq.h:367: B is computed once per step() from the last accepted evaluation), not the
    # delta optCallBack has moved to since.  Golden: the real solver, same analytic Jacobian.
    ds, g = load_golden("g1_cfg2_huber_retry")
    o = ol.Oracle(ds, with_huber=True)
    prm = aar.lm_default_params(tau=float(g["tau"][0]))
    with Problem(ds, with_huber=True) as p:
        x, rep = p.lm_solve(ds.x_full, params=prm, trace_cap=600)
    xo, repo = o.lm_solve(ds.x_full, params=ol.mapper_params(tau=float(g["tau"][0])), jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
    tries = [t["tries"] for t in rep["trace"]]
    assert max(tries) > 1 and tries[:60] == [t["tries"] for t in repo["trace"]][:60]      # the port records the tries, the reference does not
    k = 60                                                                                # well past the retry, before 500 steps of rounding pile up
    np.testing.assert_allclose([t["err"] for t in rep["trace"]][:k], g["analytic_err"][:k], rtol=1e-6)
    # mu follows (2 rho - 1)^3 of a gain ratio whose numerator is a difference of two nearly equal errors: the order of the fp64
    # atomics moves it in the fifth digit between runs (seen: 1.8e-5)
    np.testing.assert_allclose([t["mu"] for t in rep["trace"]][:k], g["analytic_mu"][:k], rtol=2e-4)
    assert abs(rep["iterations"] - int(g["analytic_iterations"][0])) <= 2
    rmse = np.sqrt(rep["final_err"] / (4 * ds.num_obs))
    assert abs(rmse - np.sqrt(float(g["analytic_final_err"][0]) / (4 * ds.num_obs))) < 1e-4


def test_600_entities_take_the_mfma_schur_path_and_match_the_oracle(monkeypatch):
    # 4 cameras + 596 markers: more shared entities than the output-stationary Schur kernel's LDS row panel holds (~560); the
    # limit is that kernel's alone -- the dense-panel MFMA kernel (default from 96 entities) solves the problem, 38 tiles of LDL^T
    ds = aar.synth(3, num_cams=4, num_markers=596, num_frames=24)
    o = ol.Oracle(ds)
    with Problem(ds) as p:
        r, ss = p.eval_residuals(ds.x_full)
        assert np.array_equal(r, o.residuals(ds.x_full, res_mode=ol.RES_F32))
        for mu in (1e5, 1e2):
            d = p.eval_damped_step(ds.x_full, mu)
            do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-8, mu
        x, rep = p.lm_solve(ds.x_full)
        assert rep["iterations"] < 60 and rep["final_err"] < rep["initial_err"]
    # ... and when the dense panels do not fit the memory budget the problem is refused (A > 560), while a problem the other
    # kernel can hold falls back to it silently and gives the same step
    monkeypatch.setenv("AAR_SCHUR_PANEL_MB", "0")
    with pytest.raises(aar.AarError) as e:
        Problem(ds)
    assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    ds2 = aar.synth(3, num_cams=4, num_markers=120, num_frames=24)
    with Problem(ds2) as p:       # budget 0 -> output-stationary kernel
        d_os = p.eval_damped_step(ds2.x_full, 1e3)
    monkeypatch.delenv("AAR_SCHUR_PANEL_MB")
    with Problem(ds2) as p:       # default: MFMA kernel (A = 124 >= 96)
        d_mf = p.eval_damped_step(ds2.x_full, 1e3)
    assert np.abs(d_os - d_mf).max() / np.abs(d_mf).max() < 1e-9


def test_reference_shaped_solver_calls_compile_and_run_against_the_mirror(tmp_path):
    # tests/tools/solver_seam_main.cpp: caller code in the shape of libs/multicam_mapper.cpp:419-443 -- solver.solve(io_vec,
    # bind(&MultiCamMapper::error_function, ...), bind(&MultiCamMapper::jacobian_function, ...)), init(z, f) / step(f, J) / step(f),
    # solve(z, bind(&MultiCamMapper::error_function_tracking, ...)) -- against aar::SparseLevMarq<double> / aar::MultiCamMapper
    import subprocess
    from conftest import PKG, ROOT
    exe = str(tmp_path / "solver_seam_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "solver_seam_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, "2"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = dict(l.split(" = ") for l in run.stdout.splitlines() if " = " in l)
    ds = aar.synth(2)
    # the reference-shaped call from outside the class is the mirror's own solve(): same iterations, same error, same z
    assert int(kv["shaped_iterations"]) == int(kv["own_iterations"]) > 3
    np.testing.assert_allclose(float(kv["shaped_final_err"]), float(kv["own_final_err"]), rtol=1e-9)
    assert float(kv["shaped_return"]) == float(kv["shaped_final_err"]) and float(kv["shaped_vs_own_max_abs_z"]) < 1e-7
    assert "initial_error: " in run.stdout and "error size: %d" % (8 * ds.num_obs) in run.stdout        # libs/multicam_mapper.cpp:424
    # step-by-step: four steps from the start equal the first four iterations of a solve
    with Problem(ds, with_huber=False) as p:
        _, rep = p.lm_solve(ds.x_full, params=aar.lm_default_params(max_iters=4), trace_cap=8)
    assert int(kv["steps_accepted"]) == 4 and int(kv["steps_zlen"]) == ds.full_len
    np.testing.assert_allclose(float(kv["steps_err"]), rep["trace"][3]["err"], rtol=1e-7)
    # verbose: the reference's two lines per step, with its stage names (libs/sparselevmarq.h:421,425)
    stage = [l for l in run.stderr.splitlines() if l.startswith(" J=")]
    assert len(stage) == 2 and all(k in stage[0] for k in (" transpose=", " Jt*J=", " B=", " chol="))
    assert sum(l.startswith("Curr Error=") and "dumping factor=" in l for l in run.stderr.splitlines()) == 2
    vals = dict(t.split("=") for t in stage[0].split())
    assert float(vals["J"]) > 0 and float(vals["chol"]) > 0 and float(vals["Jt*J"]) > 0
    # a caller's own evaluation function runs on the host loop of the same solver object (tests/test_host_levmarq.py holds that loop against the reference's
    # solver); a host function mixed with a mapper function is refused, mismatched owners too; the Jacobian function is not callable by hand; a solver whose
    # device problem was destroyed by a Config change says so instead of using freed memory
    assert kv["host_callback"] == "solved" and int(kv["host_callback_calls"]) > 10 and float(kv["host_callback_err"]) < 1e-12
    assert np.allclose([float(t) for t in kv["host_callback_z"].split()], [1.0, -0.5], atol=1e-6) and kv["mixed_host_device"] == "logic_error"
    assert kv["mixed_owners"] == "logic_error" and kv["direct_jacobian"] == "logic_error" and kv["stale_step"] == "runtime_error"
    # track() in the reference's shape: every frame refined, z = the frame poses
    assert int(kv["track_frames"]) == ds.num_frames and int(kv["track_zlen"]) == 6 * ds.num_frames and float(kv["track_max_err"]) < 100.0


def _det_run(ds, det, with_huber=False, intrinsics=False, **solve_kw):
    with Problem(ds, with_huber=with_huber, intrinsics=intrinsics, deterministic=det) as p:
        x0 = p.x_with_intrinsics(ds.x_full) if intrinsics else ds.x_full
        H, B, ss = p.eval_normal_equations(x0)
        d = p.eval_damped_step(x0, 1e3)
        x, rep = p.lm_solve(x0, trace_cap=600, **solve_kw)
    return [H, B, d, x, np.array([t["err"] for t in rep["trace"]]), np.array([t["mu"] for t in rep["trace"]])]


@pytest.mark.parametrize("name,kw", [("g1_cfg2", {}), ("g1_cfg2_huber", {"with_huber": True}), ("g1_cfg2_intr", {"intrinsics": True}), ("g1_cfg3_cut", {})])
def test_deterministic_mode_gives_the_same_bits_twice(name, kw):
    # aar_solver_options.deterministic (csrc/kernels.h): every sum the default path leaves to fp64 atomics is taken in a fixed order, as the
    # reference's ascending-row accumulation is (libs/sparselevmarq.h:291-303).  Normal equations, a damped step, the solution and
    # the whole LM trace (505 steps with -with-huber) come out bit-identical in two runs -- and agree with the default path.
    ds, g = load_golden(name)
    a, b = _det_run(ds, True, **kw), _det_run(ds, True, **kw)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    c = _det_run(ds, False, **kw)
    assert np.abs(a[0] - c[0]).max() / np.abs(c[0]).max() < 1e-14 and np.abs(a[1] - c[1]).max() / np.abs(c[1]).max() < 1e-12
    assert np.abs(a[2] - c[2]).max() / np.abs(c[2]).max() < 1e-9
    n = len(g["analytic_err"])
    assert len(a[4]) == n
    np.testing.assert_allclose(a[4], g["analytic_err"], rtol=1e-6)        # (505 steps: 2.2e-7 observed; 1e-5 is the bar of the default path)
    if n < 100:
        np.testing.assert_allclose(a[5], g["analytic_mu"], rtol=1e-9)


def test_deterministic_mode_tightens_the_retry_trace():
    # the same run as test_huber_schedule_with_a_rejected_try: with fixed-order sums the damping follows the real solver's to
    # 1e-8 over the first 60 steps (2e-4 is what the default path's atomics allow: their order moves mu between runs)
    ds, g = load_golden("g1_cfg2_huber_retry")
    prm = aar.lm_default_params(tau=float(g["tau"][0]))
    with Problem(ds, with_huber=True, deterministic=True) as p:
        x, rep = p.lm_solve(ds.x_full, params=prm, trace_cap=600)
    k = 60
    assert max(t["tries"] for t in rep["trace"]) > 1
    # (observed: 2.7e-10 with the observation passes in wrench form, 6e-12 in row form -- the same blocks, products associated differently;
    #  scripts/dev/det_margin.py prints it)
    np.testing.assert_allclose([t["mu"] for t in rep["trace"]][:k], g["analytic_mu"][:k], rtol=1e-8)
    np.testing.assert_allclose([t["err"] for t in rep["trace"]][:k], g["analytic_err"][:k], rtol=1e-6)
    n = min(len(rep["trace"]), len(g["analytic_err"]))
    np.testing.assert_allclose([t["err"] for t in rep["trace"]][:n], g["analytic_err"][:n], rtol=2e-6)
    assert rep["iterations"] == int(g["analytic_iterations"][0])


def test_deterministic_mode_on_a_many_entity_problem():
    # 124 shared entities: the default path would take the MFMA Schur kernel; deterministic mode keeps the output-stationary one
    # (fixed-order sums exist for it only) -- same step to rounding, same bits twice; beyond its LDS row panel the mode is refused
    ds = aar.synth(3, num_cams=4, num_markers=120, num_frames=24)
    with Problem(ds, deterministic=True) as p:
        d1 = p.eval_damped_step(ds.x_full, 1e3)
        assert p.solver_stats()["deterministic"]
    with Problem(ds, deterministic=True) as p:
        d2 = p.eval_damped_step(ds.x_full, 1e3)
    with Problem(ds) as p:
        d0 = p.eval_damped_step(ds.x_full, 1e3)
        assert not p.solver_stats()["deterministic"]
    assert np.array_equal(d1, d2) and np.abs(d1 - d0).max() / np.abs(d0).max() < 1e-9
    with pytest.raises(aar.AarError) as e:
        Problem(aar.synth(3, num_cams=4, num_markers=596, num_frames=24), deterministic=True)
    assert e.value.code == aar.AAR_ERR_UNSUPPORTED


def test_pcg_solver_mode_against_the_direct_path():
    # aar_solver_options.solver = AAR_SOLVER_PCG (csrc/pcg_kernels.hip): the reduced system by preconditioned CG through the frame blocks.  At a tight
    # tolerance its damped step IS the direct step (and the oracle's); at the default forcing term (eta = 0.1) the LM run is inexact
    # Newton -- another trajectory to the same fixed point: final RMSE within the north star's 1e-4 px (observed: 1e-6), no more LM steps
    ds = aar.synth(3, num_frames=120)
    o = ol.Oracle(ds)
    with Problem(ds) as p:
        d_direct = p.eval_damped_step(ds.x_full, 1e3)
        x_d, rep_d = p.lm_solve(ds.x_full)
        rmse_d, _ = p.reproj_stats(x_d)
        assert p.pcg_iterations() == (0, 0)
    with Problem(ds, solver="pcg", pcg_eta=1e-11) as p:
        d_pcg = p.eval_damped_step(ds.x_full, 1e3)
        last, total = p.pcg_iterations()
        assert 5 < last == total < 200
    do = o.damped_solve(ds.x_full, 1e3, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
    assert np.abs(d_pcg - d_direct).max() / np.abs(d_direct).max() < 1e-7
    assert np.abs(d_pcg - do).max() / np.abs(do).max() < 1e-7
    for opt in ((True, True, True), (False, True, True), (True, False, True)):      # gauge / switched-off groups are identity rows of the operator
        with Problem(ds, optimize=opt, solver="pcg") as p:
            assert p.solver_stats()["pcg_eta"] == 5e-3 and p.solver_stats()["pcg_eta_loose"] == 0.0
            x_p, rep_p = p.lm_solve(ds.x_full)
            rmse_p, _ = p.reproj_stats(x_p)
            its = p.pcg_iterations()[1]
        if opt == (True, True, True):
            assert abs(rmse_p - rmse_d) < 1e-6
            assert rep_p["iterations"] <= rep_d["iterations"] + 1 and 0 < its < 60 * rep_p["iterations"]
        else:
            with Problem(ds, optimize=opt) as q:
                x_q, _ = q.lm_solve(ds.x_full)
                rmse_q, _ = q.reproj_stats(x_q)
            assert abs(rmse_p - rmse_q) < 1e-4
    # the reference's default Config (intrinsics entities are shared entities like any other) and -with-huber go through the same operator
    with Problem(ds, intrinsics=True, solver="pcg") as p:
        x_i, rep_i = p.lm_solve(p.x_with_intrinsics(ds.x_full))
        rmse_i, _ = p.reproj_stats(x_i)
    with Problem(ds, intrinsics=True) as q:
        x_j, rep_j = q.lm_solve(q.x_with_intrinsics(ds.x_full))
        rmse_j, _ = q.reproj_stats(x_j)
    assert abs(rmse_i - rmse_j) < 1e-4
    # frames sharded over ranks: the operator is a sum over ranks (one all-reduce of 8 n bytes per CG iteration, queued by the host between two
    # launches); same LM steps, the same solution and (almost) the same CG iteration counts as on one GPU
    # (round 6: both the one-GPU kernel and the sharded kernels carry the coarse space -- AAR_PCG_COARSE -- by the same rule: the comparison below is between two
    #  two-level preconditioned runs; block-Jacobi alone must need clearly more iterations for the same run)
    # (the one-GPU kernel keeps its coarse operator for three solves -- AAR_PCG_E_EVERY, tests/test_gpu_solvers.py -- the sharded ones form it every solve, its shares
    #  riding in the set-up's all-reduce anyway: the iteration counts are compared like for like)
    os.environ["AAR_PCG_E_EVERY"] = "1"
    try:
        with Problem(ds, solver="pcg") as p:
            x_1, rep_1 = p.lm_solve(ds.x_full)
            its_1 = p.pcg_iterations()[1]
    finally:
        del os.environ["AAR_PCG_E_EVERY"]
    os.environ["AAR_PCG_COARSE"] = "0"
    try:
        with Problem(ds, solver="pcg") as p:
            x_b, rep_b = p.lm_solve(ds.x_full)
            its_b = p.pcg_iterations()[1]
    finally:
        del os.environ["AAR_PCG_COARSE"]
    assert rep_b["iterations"] == rep_1["iterations"] and its_1 < 0.8 * its_b, (its_1, its_b)
    assert abs(rep_b["final_err"] - rep_1["final_err"]) < 2e-5 * rep_1["final_err"]
    np.testing.assert_allclose(x_b, x_1, atol=3e-5)
    def solve(comm, rank):
        with Problem(ds, comm=comm, solver="pcg") as q:
            xs, reps = q.lm_solve(ds.x_full)
            return xs, reps, q.pcg_iterations()[1]
    for world in (2, 3):
        for xs, reps, its in _run_ranks(world, solve):
            # (a rank sum in another order can move a stopping test |r| <= eta |b| by one iteration: 238 CG iterations against 240 seen)
            assert reps["iterations"] == rep_1["iterations"] and abs(its - its_1) <= 0.05 * its_1
            np.testing.assert_allclose([t["err"] for t in reps["trace"]], [t["err"] for t in rep_1["trace"]], rtol=1e-4)
            assert abs(reps["final_err"] - rep_1["final_err"]) < 2e-5 * rep_1["final_err"]     # (1.2e-6 seen = 2.5e-7 px of RMSE: an inexact solve stopped one iteration apart)
            np.testing.assert_allclose(xs, x_1, atol=3e-5)      # (two inexact runs stopped an iteration apart: the scale of the forcing term's own effect on the poses)


def test_deterministic_mode_with_two_ranks():
    # fixed-order sums rank by rank, the in-process group adds the ranks' systems in rank order: two sharded runs give the same bits
    ds, g = load_golden("g1_cfg2")
    def solve(comm, rank):
        with Problem(ds, comm=comm, deterministic=True) as q:
            return q.lm_solve(ds.x_full)
    a = _run_ranks(2, solve)
    b = _run_ranks(2, solve)
    for (xa, ra), (xb, rb) in zip(a, b):
        assert np.array_equal(xa, xb) and [t["err"] for t in ra["trace"]] == [t["err"] for t in rb["trace"]]
    assert np.array_equal(a[0][0], a[1][0])                                   # every rank holds the same solution
    np.testing.assert_allclose([t["err"] for t in a[0][1]["trace"]], g["analytic_err"], rtol=1e-7)


@pytest.mark.parametrize("mode", ["deterministic", "pcg", "spcg"])
def test_randomized_shapes_in_the_optional_modes(mode):
    # the same sweep of shapes as test_randomized_shapes_against_oracle (1-5 tiles, ragged visibility, switched-off groups, 2-3 in-process ranks
    # now and then) with deterministic sums, through the PCG solver and through the CG on the explicit reduced system at a tight tolerance
    # (whatever needs more than its 64 iterations falls back to the direct chain by itself): the damped step is the oracle's in all three
    kw = {"deterministic": dict(deterministic=True), "pcg": dict(solver="pcg", pcg_eta=1e-12, pcg_max_it=2000), "spcg": dict(solver="spcg", pcg_eta=1e-12)}[mode]
    rng = np.random.default_rng(20190221)
    done = 0
    for k in range(40):
        C, M, F = int(rng.integers(3, 11)), int(rng.integers(4, 60)), int(rng.integers(2, 160))
        try:
            ds = aar.synth(3, num_cams=C, num_markers=M, num_frames=F, seed=int(rng.integers(1, 2 ** 31)))
        except aar.AarError:
            continue
        if ds.num_obs < 20:
            continue
        opt = [(True, True, True), (True, True, True), (False, True, True), (True, False, True)][k % 4]
        o = ol.Oracle(ds, optimize=opt)
        mu = float(10.0 ** rng.integers(2, 7))
        do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        with Problem(ds, optimize=opt, **kw) as p:
            d = p.eval_damped_step(ds.x_full, mu)
            assert np.abs(d - do).max() / np.abs(do).max() < 1e-6, (mode, C, M, F, mu)
            x, rep = p.lm_solve(ds.x_full)
        xo, repo = o.lm_solve(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
        assert abs(rep["iterations"] - repo["iterations"]) <= 1, (mode, C, M, F)
        # (CG on the explicit system stops at the floor of its recurrences where 1e-12 is below it: a step good to ~1e-8, 15 of them 7e-5 of the final error at worst)
        np.testing.assert_allclose(rep["final_err"], repo["final_err"], rtol=2e-4 if mode == "spcg" else 1e-5, err_msg=str((mode, C, M, F)))
        if k % 3 == 0 and opt == (True, True, True):
            def solve(comm, rank, ds=ds):
                with Problem(ds, comm=comm, **kw) as q:
                    return q.lm_solve(ds.x_full)
            for xs, reps in _run_ranks(2 + k % 2, solve):
                assert abs(reps["iterations"] - rep["iterations"]) <= 1, (mode, C, M, F)
                np.testing.assert_allclose(reps["final_err"], rep["final_err"], rtol=1e-6)
        done += 1
        if done >= 8:
            break
    assert done >= 6


@pytest.mark.parametrize("shape", ["cfg2", "cfg3_cut", "cfg5_shaped", "few_obs_per_frame", "huber_f64", "intrinsics", "intrinsics_cfg5_shaped"])
def test_observation_passes_wrench_form_equals_row_form(shape, monkeypatch):
    # The default observation passes reach the frame blocks (V_f, g_f, W_cf, W_mf) and the shared blocks (U, g) through the observation's 6x6 Gram matrix of
    # wrenches (csrc/geom.hpp corner_wrench; csrc/eval_kernels.hip passA_wrench_body / passB_wrench_body); AAR_PASSA_WRENCH=0 keeps the row form that
    # multiplies the three 2x6 Jacobian blocks of every row (libs/multicam_mapper.cpp:976-994 in closed form).  Same algebra, different association:
    # the full normal equations, the gradient, the error and a damped step agree to rounding -- in every workgroup shape the launcher picks
    # (one / two / four lanes per observation, one or two wavefronts per frame), with the dense panels of the MFMA Schur path, in both modes.
    kw = {}
    if shape == "cfg2":
        ds = load_golden("g1_cfg2")[0]
    elif shape == "cfg3_cut":
        ds = load_golden("g1_cfg3_cut")[0]
    elif shape == "cfg5_shaped":
        ds = aar.synth(5, num_frames=40)                      # 16 cameras / 200 markers: ~250 observations per frame, two wavefronts per frame, MFMA Schur panels
    elif shape == "few_obs_per_frame":
        ds = aar.synth(3, num_cams=3, num_markers=6, num_frames=60)   # <= 14 observations per frame: four lanes per observation
    elif shape == "huber_f64":
        ds = load_golden("g1_cfg2_huber")[0]
        kw = dict(with_huber=True, residual_mode=aar.RES_F64)
    elif shape == "intrinsics":                               # optimize_cam_intrinsics: the intrinsics entities' slots collect sum G_k^T w^T
        ds = load_golden("g1_cfg2_intr")[0]
        kw = dict(intrinsics=True)
    else:
        ds = aar.synth(5, num_frames=30)
        kw = dict(intrinsics=True)
    x_eval = None
    out = {}
    for form in ("1", "0"):   # "1": the default (inside the merged launch of a small problem pass B's chunks stay in row form)
        monkeypatch.setenv("AAR_PASSA_WRENCH", form)
        for det in (False, True):
            with Problem(ds, deterministic=det, solver="direct", **kw) as p:
                x_eval = p.x_with_intrinsics(ds.x_full) if kw.get("intrinsics") else ds.x_full
                H, B, ss = p.eval_normal_equations(x_eval)
                d = p.eval_damped_step(x_eval, 1e2)
            out[form, det] = (H, B, ss, d)
    for det, form in ((False, "1"), (True, "1")):
        (H1, B1, s1, d1), (H0, B0, s0, d0) = out[form, det], out["0", det]
        assert np.abs(H1 - H0).max() / np.abs(H0).max() < 1e-13
        assert np.abs(B1 - B0).max() / np.abs(B0).max() < 1e-12
        assert abs(s1 - s0) <= 1e-13 * s0
        assert np.abs(d1 - d0).max() / np.abs(d0).max() < 1e-8        # (the small problem is the ill-conditioned one: 1.5e-9; the others 1e-11)
    # the deterministic mode of the wrench form gives the same bits twice
    monkeypatch.setenv("AAR_PASSA_WRENCH", "1")
    with Problem(ds, deterministic=True, solver="direct", **kw) as p:
        H, B, ss = p.eval_normal_equations(x_eval)
    assert np.array_equal(H, out["1", True][0]) and np.array_equal(B, out["1", True][1]) and ss == out["1", True][2]


@pytest.mark.gpu
def test_one_thread_drives_problems_on_two_devices():
    """the page-locked staging of csrc/hostcopy.hip keeps two events per host thread; an event belongs to ONE device, so a thread that uploads to
    device 0 and then to device 1 must get events of device 1 (skipped on a one-GPU box: the pool's boxes have one)."""
    if aar.device_count() < 2:
        pytest.skip("needs two GPUs")
    ds = aar.synth(2)
    with aar.Problem(ds, device=0) as p0, aar.Problem(ds, device=1) as p1:
        x0, r0 = p0.lm_solve(ds.x_full)
        x1, r1 = p1.lm_solve(ds.x_full)
        x0b, _ = p0.lm_solve(ds.x_full)
    assert r0["iterations"] == r1["iterations"] and np.allclose(x0, x1, atol=1e-9) and np.allclose(x0, x0b, atol=1e-9)
