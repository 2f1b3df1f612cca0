"""CPU pins of tests/track_restated.py, the float64 restatement tests/test_gpu_track.py holds k_track to.

The restatement shares no code with the oracle: its complex-step Jacobian must equal the oracle's analytic frame block, its Huber
Jacobian the central differences of its own weighted residual, and its LM loop the oracle's restated SparseLevMarq (plain residuals)
and the real solver's golden track() run (Huber).
"""
import numpy as np
import pytest

import oracle_lib as ol
import track_restated as tr
from conftest import load_golden


def _track_ds(name):
    ds, g = load_golden(name)
    ds.x_full = np.array(g["track_x0"])
    return ds, g


def test_complex_step_jacobian_equals_the_oracle_frame_block():
    ds, g = _track_ds("g_track_cfg2")
    td = tr.TrackData(ds, ds.x_full)
    worst = 0.0
    for f in range(ds.num_frames):
        sub = ol.frame_subproblem(ds, f)
        if sub.num_obs == 0:
            continue
        o = ol.Oracle(sub, optimize=(False, False, True))
        rows, cols, vals = o.jacobian(sub.x_full, jac_mode=ol.JAC_ANALYTIC)
        Jo = np.zeros((8 * sub.num_obs, 6))
        np.add.at(Jo, (rows, cols), vals)
        fd = td.frame(f)
        J, r = tr.jacobian(fd, td.z0[f], -1.0)
        # same residual rows (the oracle's double-mode residuals) and the same derivative of them
        np.testing.assert_allclose(r, o.residuals(sub.x_full, res_mode=ol.RES_F64), rtol=0, atol=1e-9)
        worst = max(worst, np.abs(J - Jo).max() / np.abs(Jo).max())
    assert worst < 1e-12, worst


def test_rodrigues_at_zero_keeps_the_first_order_term():
    # theta = 0 exactly: R(i h e_k) = I + i h [e_k]x to first order, so the complex step sees d R / d w_k = [e_k]x
    for k in range(3):
        w = np.zeros(3, dtype=complex)
        w[k] = 1j * tr.H_CS
        e = np.zeros(3)
        e[k] = 1.0
        np.testing.assert_array_equal(tr.rodrigues(w).imag / tr.H_CS, tr.hat(e))
        np.testing.assert_array_equal(tr.rodrigues(w).real, np.eye(3))


@pytest.mark.parametrize("delta", [10.0, 1.0])
def test_weighted_jacobian_matches_central_differences(delta):
    ds, g = _track_ds("g_track_cfg2_huber")
    td = tr.TrackData(ds, ds.x_full)
    outliers, inliers, worst = 0, 0, 0.0
    hstep = 1e-6
    for f in range(ds.num_frames):
        fd = td.frame(f)
        if fd["ou"].shape[0] == 0:
            continue
        z = td.z0[f]
        J, _ = tr.jacobian(fd, z, delta)
        Jn = np.zeros_like(J)
        for k in range(6):
            e = np.zeros(6)
            e[k] = hstep
            rp, _ = tr.weighted(fd, z + e, delta)
            rm, _ = tr.weighted(fd, z - e, delta)
            Jn[:, k] = (rp - rm).reshape(-1) / (2 * hstep)
        _, out = tr.weighted(fd, z, delta)
        outliers += int(out.sum())
        inliers += int((~out).sum())
        worst = max(worst, np.abs(J - Jn).max() / np.abs(J).max())
        # the weight's derivative is there: the plain Jacobian times w differs from it on the outlier corners
        if out.any():
            J0, r0 = tr.jacobian(fd, z, -1.0)
            w, _ = tr.huber_weights(tr.residuals(fd, z), delta)
            Jw = J0 * np.repeat(w.reshape(-1), 2)[:, None]
            assert np.abs(Jw - J).max() > 1e-6 * np.abs(J).max()
    assert outliers > 0 and inliers > 0, (outliers, inliers)
    assert worst < 1e-6, worst


def test_restated_lm_equals_the_oracle_on_every_frame():
    ds, g = _track_ds("g_track_cfg2")
    ns = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    x, res = tr.track_all(ds, ds.x_full)
    for f, r in enumerate(res):
        sub = ol.frame_subproblem(ds, f)
        o = ol.Oracle(sub, optimize=(False, False, True))
        xs, rep = o.lm_solve(sub.x_full, params=ol.mapper_params(huber_fixed=1), jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)
        assert r["iterations"] == rep["iterations"], f
        np.testing.assert_allclose(r["err"], rep["final_err"], rtol=1e-10)
        assert np.abs(r["z"] - xs[ns:ns + 6]).max() < 1e-10, f
    assert np.array_equal(x[:ns], ds.x_full[:ns])


def test_restated_lm_with_huber_meets_the_real_solver():
    # the same bars as tests/test_gpu_parity.py::test_track_frames_vs_real_solver holds the kernel to (the golden's Jacobian is the
    # real solver's central differences, delta 1e-3)
    ds, g = _track_ds("g_track_cfg2_huber")
    ns = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    x, res = tr.track_all(ds, ds.x_full, delta=10.0)
    it = np.array([r["iterations"] for r in res])
    err = np.array([r["err"] for r in res])
    np.testing.assert_allclose(err, g["track_err"], rtol=1e-5, atol=1e-6)
    assert np.abs(x[ns:] - g["track_x"][ns:]).max() < 2e-4
    assert np.abs(it - g["track_iterations"]).max() <= 1 and np.mean(it == g["track_iterations"]) > 0.9
    assert sum(r["outliers"] for r in tr.track_all(ds, ds.x_full, delta=10.0, max_iters=0)[1]) > 0


def test_decision_margin_and_exits_on_small_cases():
    ds, g = _track_ds("g_track_cfg2")
    td = tr.TrackData(ds, ds.x_full)
    fd = td.frame(0)
    # a frame with no detection does nothing
    empty = {k: v[:0] for k, v in fd.items()}
    r = tr.track_frame(empty, td.z0[0])
    assert r["iterations"] == 0 and r["err"] == 0.0 and np.array_equal(r["z"], td.z0[0]) and r["margin"] == np.inf
    # the iteration cap and a large min_error (exit 1 after the first accepted step)
    assert tr.track_frame(fd, td.z0[0], max_iters=1)["iterations"] == 1
    r = tr.track_frame(fd, td.z0[0], min_error=1e30)
    assert r["iterations"] == 1 and r["exit"] == 1
    # zero residuals exactly: gain 0/0, no accepted try, exit 2 after one iteration, the pose untouched
    zr = dict(fd)
    zr["ou"] = fd["ou"] - tr.residuals(fd, td.z0[0])
    assert np.abs(tr.residuals(zr, td.z0[0])).max() == 0.0
    r = tr.track_frame(zr, td.z0[0])
    assert r["iterations"] == 1 and r["exit"] == 2 and r["err"] == 0.0 and np.array_equal(r["z"], td.z0[0]) and r["rejected"] == 1
