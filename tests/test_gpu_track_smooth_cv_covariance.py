"""Pose covariance of constant-velocity smoothed tracks (aar_track_smooth_covariance2): the diagonal, lag-one and lag-two
blocks of H^-1 from the device's downward pass over the supernode cyclic reduction's elimination tree.  Needs a real MI355X.

Yardstick: numpy.linalg.inv of the dense H built from the blocks aar_track_smooth_system2 returned at mu = 0 (the assembly is certified by
tests/test_gpu_track_smooth_cv.py).  Bar (frame_cov, lag_cov, lag2_cov alike): largest entry error over the largest entry of the yardstick's
selected blocks <= 10 eps kappa_2(H), the forward-error order of any inverse (section 28's bar).  At 2000 frames columns of the inverse from
scipy.linalg.solveh_banded on unit right-hand sides take the dense inverse's place, with kappa_2 from scipy.linalg.eigvals_banded.
Block rows: sum_j H_fj Sigma_jf = I for every frame from the outputs alone, normalised by sum_j |H_fj|_2 |Sigma_jf|_2, held to
100 x NUMPY_BLOCK_ROW = the largest value numpy's own inverse reaches at F = 4, 131 and 500 (on the restated systems of the same inputs,
measured on the CPU: 3.67e-16, 1.60e-15, 4.59e-16; DESIGN.md section 32 has the table).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.linalg import eigvals_banded, solveh_banded

import aar
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_cv_covariance_restated as ccr
import smooth_cv_restated as cv
import track_restated as tr
from conftest import GOLDEN, PKG, ROOT, load_golden
from test_gpu_live_marginal import parse_live_cov_yaml

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SROT, STRANS = cc.SROT, cc.STRANS
CV = dict(model="cv", sigma_rot0=cc.SROT0, sigma_trans0=cc.STRANS0)
T = 16                       # SMOOTH_CV_T of csrc/kernels.h
NUMPY_BLOCK_ROW = 1.60e-15
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 66, 129, 131]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _dataset(F):
    """config 2 cut to F frames with the frames of sc.emptied(F) emptied"""
    ds = sc.without_frames(aar.synth(2, num_frames=F), sc.emptied(F))
    assert ds.num_frames == F
    return ds


def _own_levels(F):
    K, n, s = (F + 1) // 2, 0, 1
    while s < K and -(-K // (2 * s)) > T:
        n, s = n + 1, 2 * s
    return n


def _launches(F):
    """the evaluation (2), the solve (1, or 2 + 2 per own level), the downward pass (the tail, one per own level, the unpacking)"""
    n = _own_levels(F)
    return 2 + (2 * n + 2 if n else 1) + (2 + n)


def _kappa(H):
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    return float(ev[-1] / ev[0])


def _against_the_inverse(tag, gd, go, go2, got):
    F = gd.shape[0]
    H = cv.dense(gd, go, go2)
    kappa = _kappa(H)
    want = ccr.selected_blocks(np.linalg.inv(H), F)
    big = max(np.abs(w).max() for w in want if w.size)
    errs = [float(np.abs(g - w).max() / big) if w.size else 0.0 for g, w in zip(got, want)]
    print("%s: kappa %.3e, frame_cov %.2e lag_cov %.2e lag2_cov %.2e = %.4f / %.4f / %.4f eps kappa; block rows: numpy %.2e" %
          ((tag, kappa) + tuple(errs) + tuple(e / (EPS * kappa) for e in errs) + (ccr.block_row_residual(gd, go, go2, *want),)))
    assert max(errs) <= 10 * EPS * kappa, (errs, 10 * EPS * kappa)
    return kappa


def _check_report(rep, ds, cost, F):
    assert rep["num_residuals"] == 8 * ds.num_obs + 6 * max(F - 1, 0) and rep["num_vars"] == 6 * F
    assert (rep["data_cost"], rep["prior_cost"]) == cost
    dof = rep["num_residuals"] - rep["num_vars"]
    np.testing.assert_allclose(rep["sigma2"], (cost[0] + cost[1]) / dof if dof > 0 else 0.0, rtol=1e-15)
    assert rep["launches"] == _launches(F) and rep["seconds"] > 0


# ---- 1. blocks against the inverse, every launch shape ----
@pytest.mark.parametrize("F", SIZES)
def test_blocks_against_the_inverse(F):
    ds = _dataset(F)
    x0 = sc.track_start(ds)
    ft = cc.gaps(F) if F > 1 else None
    with aar.Problem(ds) as p:
        gd, go, go2, _, _, cost = p.track_smooth_system2(x0, SROT, STRANS, 0.0, frame_time=ft, **CV)
        S, R, R2, rep = p.track_smooth_covariance2(x0, SROT, STRANS, frame_time=ft, **CV)
    assert S.shape == (F, 6, 6) and R.shape == (max(F - 1, 0), 6, 6) and R2.shape == (max(F - 2, 0), 6, 6)
    _against_the_inverse("F %d" % F, gd, go, go2, (S, R, R2))
    rows = ccr.block_row_residual(gd, go, go2, S, R, R2)
    print("F %d: block rows: device %.2e (launches %d)" % (F, rows, rep["launches"]))
    assert rows <= 100 * NUMPY_BLOCK_ROW, rows
    assert np.array_equal(S, np.swapaxes(S, 1, 2))
    _check_report(rep, ds, cost, F)
    assert [_own_levels(n) for n in (4 * T, 4 * T + 1, 8 * T, 8 * T + 1)] == [0, 1, 1, 2]


def test_columns_at_two_thousand_frames():
    F = 2000
    ds = _dataset(F)
    x0 = sc.track_start(ds)
    ft = cc.gaps(F)
    with aar.Problem(ds) as p:
        gd, go, go2, _, _, cost = p.track_smooth_system2(x0, SROT, STRANS, 0.0, frame_time=ft, **CV)
        S, R, R2, rep = p.track_smooth_covariance2(x0, SROT, STRANS, frame_time=ft, **CV)
    n0 = _own_levels(F)
    assert n0 == 5                                   # the finishing workgroup starts at stride 32: supernodes 32 m, frames 64 m and 64 m + 1
    # both ends, an emptied frame, both sides of each launch boundary: supernodes 7 | 9 (two workgroups of the stride-1 launch), 16 (the
    # launch of stride 16), 31 | 32 | 33 (stride 1, the finishing workgroup, stride 1), 512 (the top stride)
    frames = [0, 1, 14, 18, 32, 63, 64, 66, F // 3 + 5, 1024, F - 2, F - 1]
    assert F // 3 + 5 in sc.emptied(F)
    ab = cv.banded(gd, go, go2)
    n = 6 * F
    ev = eigvals_banded(ab, lower=True)            # (one reduction to tridiagonal form for both ends of the spectrum)
    assert ev[0] > 0
    kappa = float(ev[-1] / ev[0])
    E = np.zeros((n, 6 * len(frames)))
    for k, f in enumerate(frames):
        E[6 * f:6 * f + 6, 6 * k:6 * k + 6] = np.eye(6)
    X = solveh_banded(ab, E, lower=True)
    big, err = 0.0, 0.0
    for k, f in enumerate(frames):
        col = X[:, 6 * k:6 * k + 6].reshape(F, 6, 6)          # col[j] = Sigma_jf
        pairs = [(S[f], col[f])]
        if f + 1 < F:
            pairs.append((R[f], col[f + 1].T))
        if f + 2 < F:
            pairs.append((R2[f], col[f + 2].T))
        if f >= 1:
            pairs.append((R[f - 1], col[f - 1]))
        if f >= 2:
            pairs.append((R2[f - 2], col[f - 2]))
        for got, ref in pairs:
            big = max(big, float(np.abs(ref).max()))
            err = max(err, float(np.abs(got - ref).max()))
    print("F %d: kappa %.3e, %d frames' columns: %.2e = %.4f eps kappa" % (F, kappa, len(frames), err / big, err / big / (EPS * kappa)))
    assert err / big <= 10 * EPS * kappa, (err / big, 10 * EPS * kappa)
    rows = ccr.block_row_residual(gd, go, go2, S, R, R2)
    print("F %d: block rows: device %.2e (launches %d)" % (F, rows, rep["launches"]))
    assert rows <= 100 * NUMPY_BLOCK_ROW, rows
    assert np.array_equal(S, np.swapaxes(S, 1, 2))
    _check_report(rep, ds, cost, F)


# ---- 2. properties ----
def test_properties():
    F = 65
    ds = _dataset(F)
    empty = sc.emptied(F)
    assert empty == [0] + list(range(21, 31)) + [64]
    x0 = sc.track_start(ds)
    ft = cc.gaps(F)
    keep = np.array(x0)
    with aar.Problem(ds) as p:
        a0 = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
        S, R, R2, rep = p.track_smooth_covariance2(x0, SROT, STRANS, frame_time=ft, **CV)
        Sb, Rb, R2b, repb = p.track_smooth_covariance2(x0, SROT, STRANS, frame_time=ft, **CV)
        a1 = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
    assert np.array_equal(x0, keep)                                   # x_full is not modified
    assert np.array_equal(S, Sb) and np.array_equal(R, Rb) and np.array_equal(R2, R2b)      # two calls give identical bits
    for k in ("num_residuals", "num_vars", "data_cost", "prior_cost", "sigma2", "launches"):
        assert rep[k] == repb[k], k
    for u, v in zip(a0, a1):                                          # aar_track_smooth before and after: the same bits
        if isinstance(u, dict):
            for k in u:
                assert k == "seconds" or u[k] == v[k], k
        else:
            assert np.array_equal(u, v)
    assert np.array_equal(S, np.swapaxes(S, 1, 2))                    # the kernel mirrors the lower triangle: symmetric to the bit
    assert all(np.all(np.isfinite(a)) for a in (S, R, R2))
    assert min(np.linalg.eigvalsh(S[f])[0] for f in range(F)) > 0
    D2 = np.hstack([np.eye(6), -2 * np.eye(6), np.eye(6)])            # z_{f+2} - 2 z_{f+1} + z_f
    lo18, lo2 = np.inf, np.inf
    for f in range(F - 2):
        M = np.block([[S[f], R[f], R2[f]], [R[f].T, S[f + 1], R[f + 1]], [R2[f].T, R[f + 1].T, S[f + 2]]])
        lo18 = min(lo18, np.linalg.eigvalsh(0.5 * (M + M.T))[0])
        C2 = D2 @ M @ D2.T
        lo2 = min(lo2, np.linalg.eigvalsh(0.5 * (C2 + C2.T))[0])
    print("smallest eigenvalue: three-frame blocks %.3e, second differences %.3e" % (lo18, lo2))
    assert lo18 > 0 and lo2 > 0
    # a frame without detections is carried by its neighbours: finite, and less certain than the observed frames around it
    cnt = np.bincount(ds.obs_frame, minlength=F)
    assert np.all(cnt[empty] == 0)
    tvar = np.einsum("fii->f", S[:, 3:, 3:])
    run = [f for f in empty if 0 < f < F - 1]
    left, right = run[0] - 1, run[-1] + 1
    assert cnt[left] > 0 and cnt[right] > 0 and cnt[1] > 0 and cnt[F - 2] > 0
    for f in run:
        assert tvar[f] > tvar[left] and tvar[f] > tvar[right], f
    assert tvar[0] > tvar[1] and tvar[F - 1] > tvar[F - 2]
    print("translation variance (unscaled): ends %.3e %.3e against %.3e %.3e; gap's neighbours %.3e %.3e, emptied run %s" %
          (tvar[0], tvar[F - 1], tvar[1], tvar[F - 2], tvar[left], tvar[right], np.array2string(tvar[run], precision=3)))


# ---- 3. consistency with the estimator ----
def test_consistency_with_the_estimator():
    """Measured on the MI355X: see DESIGN.md section 32 for the recorded value."""
    ds, x0, empty = cc.claim_case()
    F = ds.num_frames
    n0 = sc.ns(ds)
    zt = np.asarray(ds.x_truth)[n0:n0 + 6 * F].reshape(F, 6)
    prm = aar.lm_default_params(min_average_step_error_diff=cc.TIGHT["min_avg"], max_iters=cc.TIGHT["max_iters"])
    with aar.Problem(ds) as p:
        xs, srep, _, _ = p.track_smooth(x0, SROT, STRANS, params=prm, **CV)
        S, R, R2, rep = p.track_smooth_covariance2(xs, SROT, STRANS, **CV)
    td = tr.TrackData(ds, x0)
    sp = cv.SmoothCvProblem(td, SROT, STRANS, cc.SROT0, cc.STRANS0)
    r = cv.smooth_lm(sp, td.z0, **cc.TIGHT)
    assert r["margin"] > 1e-9 and srep["iterations"] == r["iterations"]
    diag, off, off2, _ = sp.system(r["z"])
    Sd = ccr.selected_blocks(np.linalg.inv(cv.dense(diag, off, off2)), F)[0]
    rows = 8 * ds.num_obs + 6 * (F - 1)
    sigma2 = r["err"] / (rows - 6 * F)

    def mahalanobis(z, s2, blocks):
        d = z.reshape(F, 6) - zt
        return float(np.mean([d[f] @ np.linalg.solve(s2 * blocks[f], d[f]) for f in range(F)]))
    m_dev = mahalanobis(xs[n0:n0 + 6 * F], rep["sigma2"], S)
    m_ref = mahalanobis(r["z"], sigma2, Sd)
    print("claim case: sigma2 %.6e (restated %.6e); mean squared Mahalanobis distance to the truth %.6f (restated %.6f); 6 would be a "
          "calibrated, independent estimate" % (rep["sigma2"], sigma2, m_dev, m_ref))
    assert abs(m_dev - m_ref) <= 1e-6 * m_ref, (m_dev, m_ref)


# ---- 4. the random walk through the new entry ----
def _raw(p, x0, F, sp_kw, frame_cov=True, lag_cov=True, lag2_cov=True, report=True, struct_size=None, fill=7.0):
    """the C call with sentinel-filled outputs: (code, frame_cov, lag_cov, lag2_cov, report struct)"""
    x = np.array(p._x(x0), dtype=np.float64)
    keep = x.copy()
    spar = aar.SmoothParams(SROT, STRANS, None, None, None, **sp_kw)
    fc, lc, l2 = np.full((max(F, 1), 6, 6), fill), np.full((max(F - 1, 1), 6, 6), fill), np.full((max(F - 2, 1), 6, 6), fill)
    rep = aar.CSmoothCovarianceReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep) if struct_size is None else struct_size
    code = aar.lib().aar_track_smooth_covariance2(p.handle, aar._dptr(x), C.byref(spar.c), aar._dptr(fc) if frame_cov else None,
                                                  aar._dptr(lc) if lag_cov else None, aar._dptr(l2) if lag2_cov else None,
                                                  C.byref(rep) if report else None)
    assert np.array_equal(x, keep)
    return code, fc, lc, l2, rep


def _golden_track(name):
    ds, g = load_golden(name)
    ds.x_full = np.array(g["track_x0"])
    return ds


def test_random_walk_through_the_new_entry():
    ds = _golden_track("g_track_cfg2")
    x0, F = ds.x_full, ds.num_frames
    ft = cc.gaps(F)
    with aar.Problem(ds) as p:
        S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS, frame_time=ft)
        S2, R2, none, rep2 = p.track_smooth_covariance2(x0, SROT, STRANS, frame_time=ft, lag2=False)
        assert none is None and np.array_equal(S, S2) and np.array_equal(R, R2)
        for k in rep:
            assert k == "seconds" or rep[k] == rep2[k], k
        code, fc, lc, l2, crep = _raw(p, x0, F, {})
        assert code == aar.AAR_ERR_UNSUPPORTED and "lag2_cov" in aar.lib().aar_last_error().decode()
        assert np.all(fc == 7.0) and np.all(lc == 7.0) and np.all(l2 == 7.0)
        assert bytes(bytearray(crep)[4:]) == b"\x55" * (C.sizeof(crep) - 4)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_covariance2(x0, SROT, STRANS, frame_time=ft)
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED


# ---- 5. edges and interfaces ----
@pytest.mark.parametrize("F", [6, 1])
def test_no_detection_anywhere_is_a_numeric_error(F):
    ds = sc.without_frames(aar.synth(2, num_frames=F), range(F))
    assert ds.num_obs == 0
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        code, fc, lc, l2, rep = _raw(p, x0, F, CV)
        assert code == aar.AAR_ERR_NUMERIC
        assert np.all(fc == 7.0) and np.all(lc == 7.0) and np.all(l2 == 7.0)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_covariance2(x0, SROT, STRANS, **CV)
        assert e.value.code == aar.AAR_ERR_NUMERIC


def test_null_outputs_and_truncated_report():
    ds = _golden_track("g_track_cfg2")
    x0, F = ds.x_full, ds.num_frames
    with aar.Problem(ds) as p:
        code, fc, lc, l2, rep = _raw(p, x0, F, CV)
        assert code == 0 and not np.any(fc == 7.0) and not np.any(lc == 7.0) and not np.any(l2 == 7.0)
        for mask in range(16):
            kw = dict(frame_cov=bool(mask & 1), lag_cov=bool(mask & 2), lag2_cov=bool(mask & 4), report=bool(mask & 8))
            code, fc2, lc2, l22, rep2 = _raw(p, x0, F, CV, **kw)
            assert code == 0, kw
            assert np.array_equal(fc2, fc) if kw["frame_cov"] else np.all(fc2 == 7.0)
            assert np.array_equal(lc2, lc) if kw["lag_cov"] else np.all(lc2 == 7.0)
            assert np.array_equal(l22, l2) if kw["lag2_cov"] else np.all(l22 == 7.0)
            if kw["report"]:
                assert rep2.sigma2 == rep.sigma2 and rep2.num_vars == 6 * F
        # a caller compiled against a shorter report: the fields beyond its struct_size are not written
        cut = aar.CSmoothCovarianceReport.data_cost.offset
        code, _, _, _, rep3 = _raw(p, x0, F, CV, struct_size=cut)
        assert code == 0 and rep3.struct_size == cut and rep3.num_residuals == rep.num_residuals and rep3.num_vars == rep.num_vars
        assert bytes(bytearray(rep3)[cut:]) == b"\x55" * (C.sizeof(rep3) - cut)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_covariance2(x0, -1.0, STRANS, **CV)
        assert e.value.code == aar.AAR_ERR_INVALID


def test_no_frames_one_frame_two_frames():
    two = aar.synth(2, num_frames=2)
    n0 = sc.ns(two)
    z = np.zeros(0, dtype=np.int32)
    empty = sc.copy_of(two, num_frames=0, frame_ids=z, obs_frame=z, obs_cam=z, obs_marker=z, obs_uv=np.zeros((0, 8), dtype=np.float32),
                       x_full=np.array(two.x_truth[:n0]), x_truth=np.array(two.x_truth[:n0]))
    with aar.Problem(empty) as p:
        code, fc, lc, l2, rep = _raw(p, empty.x_full, 0, CV)
        assert code == 0 and np.all(fc == 7.0) and np.all(lc == 7.0) and np.all(l2 == 7.0)
        assert rep.num_vars == 0 and rep.launches == 0 and rep.sigma2 == 0.0
    one = aar.synth(2, num_frames=1)
    x0 = sc.track_start(one)
    with aar.Problem(one) as p:
        gd, _, _, _, _, cost = p.track_smooth_system2(x0, SROT, STRANS, 0.0, **CV)
        code, fc, lc, l2, rep = _raw(p, x0, 1, CV)
    Vi = np.linalg.inv(gd[0])
    assert code == 0 and np.abs(fc[0] - Vi).max() / np.abs(Vi).max() <= 10 * EPS * _kappa(gd[0])
    assert np.all(lc == 7.0) and np.all(l2 == 7.0)                  # one frame: no pair, nothing of the padded frame comes out
    assert rep.num_residuals == 8 * one.num_obs and rep.num_vars == 6 and rep.prior_cost == 0.0 and rep.launches == 5
    x0 = sc.track_start(two)
    with aar.Problem(two) as p:
        gd, go, go2, _, _, cost = p.track_smooth_system2(x0, SROT, STRANS, 0.0, **CV)
        gdr, gor, _, _, _ = p.track_smooth_system(x0, cc.SROT0, cc.STRANS0, 0.0)
        code, fc, lc, l2, rep = _raw(p, x0, 2, CV)
    assert code == 0 and np.all(l2 == 7.0) and len(go2) == 0
    assert np.abs(gd - gdr).max() <= 1e-12 * np.abs(gdr).max() and np.abs(go - gor).max() <= 1e-12 * np.abs(gor).max()   # pair 0 alone
    _against_the_inverse("two frames", gd, go, go2, (fc[:2], lc[:1], l2[:0]))


def test_unsupported_behind_a_communicator():
    ds = _golden_track("g_track_cfg2")
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            with pytest.raises(aar.AarError) as e:
                p.track_smooth_covariance2(ds.x_full, SROT, STRANS, **CV)
            assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    finally:
        comm.close()
        group.close()


def test_huber_problem():
    ds = _golden_track("g_track_cfg2_huber")
    x0 = ds.x_full
    out = {}
    for delta in (None, 1.0):
        p = aar.Problem(ds, with_huber=delta is not None)
        with p:
            if delta is not None:
                p.set_huber_delta(delta)
            gd, go, go2, _, _, _ = p.track_smooth_system2(x0, SROT, STRANS, 0.0, **CV)
            S, R, R2, rep = p.track_smooth_covariance2(x0, SROT, STRANS, **CV)
        _against_the_inverse("huber delta %s" % delta, gd, go, go2, (S, R, R2))
        out[delta] = (S, rep)
    # the Huber weights are in H and in the cost: down-weighted detections leave the poses less certain
    assert out[1.0][1]["data_cost"] < out[None][1]["data_cost"]
    assert np.einsum("fii->", out[1.0][0]) > np.einsum("fii->", out[None][0])


# ---- 6. the solve did not move ----
def test_the_solve_did_not_move():
    """tests/golden/g_smooth_cv_solve_bits.npz: recorded on the MI355X at the commit before the row helpers moved into csrc/cv_rows.hpp"""
    g = np.load(os.path.join(GOLDEN, "g_smooth_cv_solve_bits.npz"))
    ds = aar.synth(2, num_frames=40)
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        x, rep, _, _ = p.track_smooth(x0, SROT, STRANS, **CV)
    assert rep["iterations"] == int(g["iterations40"][0])
    assert np.array_equal(x[sc.ns(ds):].reshape(-1, 6), g["poses40"])
    F = 131
    ds = _dataset(F)
    x0 = sc.track_start(ds)
    ft = cc.gaps(F)
    with aar.Problem(ds) as p:
        gd = p.track_smooth_system2(x0, SROT, STRANS, 1.0, frame_time=ft, **CV)[0]
        mu0 = float(np.max(np.einsum("fii->fi", gd)))
        d = p.track_smooth_system2(x0, SROT, STRANS, mu0, frame_time=ft, **CV)[4]
    assert mu0 == float(g["mu131"][0])
    assert np.array_equal(d, g["delta131"])


# ---- 7. callers ----
def test_mapper_track_smooth_covariance_overload(tmp_path):
    exe = str(tmp_path / "smooth_cv_covariance_mapper_main")
    cc_ = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_cv_covariance_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                          "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS), repr(cc.SROT0), repr(cc.STRANS0)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = dict(l.split(" = ") for l in run.stdout.splitlines() if " = " in l)
    ds = aar.synth(2)
    F = ds.num_frames
    x0 = sc.track_start(ds)
    ft = np.asarray(ds.frame_ids, dtype=np.float64)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, _, _, _ = p.track_smooth(xt, SROT, STRANS, frame_time=ft, **CV)
        S, R, R2, rep = p.track_smooth_covariance2(xs, SROT, STRANS, frame_time=ft, **CV)
    assert int(kv["frames"]) == F and int(kv["pairs"]) == F - 1 and int(kv["lag2"]) == F - 2
    assert int(kv["num_residuals"]) == rep["num_residuals"] and int(kv["num_vars"]) == rep["num_vars"] and int(kv["launches"]) == rep["launches"]
    # (the mapper carries its poses as 4x4 matrices between its calls: a few ulps of the point; the blocks follow the point)
    np.testing.assert_allclose(float(kv["sigma2"]), rep["sigma2"], rtol=1e-7)
    for key, ref in (("S", S), ("R", R), ("Q", R2)):
        got = np.array([[float(v) for v in kv["%s%d" % (key, f)].split()] for f in range(len(ref))]).reshape(len(ref), 6, 6)
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max(), key
    assert int(kv["rw_same"]) == 1 and int(kv["rw_lag2"]) == 0


def test_find_solution_cv_covariance_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # the first 90 frames: config 2's last frames turn through pi, where the solution file's vec -> matrix -> vec round trip lands on another
    # rotation vector of the same rotation (tests/test_gpu_track_smooth_covariance.py)
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    smooth = ["-smooth", repr(SROT), repr(STRANS)]
    cvf = ["-cv", repr(cc.SROT0), repr(cc.STRANS0)]
    run = subprocess.run(base + smooth + cvf + ["-cv-covariance"], capture_output=True, text=True, timeout=300, env=dict(os.environ, AAR_DETERMINISTIC="1"))
    assert run.returncode == 0, run.stdout + run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("smooth-covariance: ")]
    assert len(line) == 1 and "smooth: constant velocity" in run.stdout, run.stdout
    y = parse_live_cov_yaml(os.path.join(folder, "final.smooth_covariance.yaml"))
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    F = got.num_frames
    assert F == FK and np.linalg.norm(got.x_full[n0:n0 + 6 * F].reshape(F, 6)[:, :3], axis=1).max() < 3.0
    with aar.Problem(got) as p:
        S, R, R2, rep = p.track_smooth_covariance2(got.x_full, SROT, STRANS, frame_time=np.asarray(got.frame_ids, dtype=np.float64), **CV)
    assert sorted(y) == sorted(int(i) for i in got.frame_ids)
    for f in range(F):
        sig, blk = y[int(got.frame_ids[f])]
        np.testing.assert_allclose(sig, rep["sigma2"], rtol=1e-6)
        assert np.abs(blk - rep["sigma2"] * S[f]).max() <= 1e-6 * np.abs(rep["sigma2"] * S[f]).max(), f
    words = line[0].replace(",", " ").split()
    s1 = np.sqrt(rep["sigma2"] * np.einsum("fii->f", S[:, 3:, 3:]))
    np.testing.assert_allclose(float(words[words.index("sigma2") + 1]), rep["sigma2"], rtol=1e-4)
    np.testing.assert_allclose([float(words[words.index("largest") + 1]), float(words[words.index("smallest") + 1])], [s1.max(), s1.min()], rtol=1e-4)
    # refused with the usage message: without -cv, without -smooth, with -live
    os.remove(os.path.join(folder, "final.smooth_covariance.yaml"))
    for bad in (base + smooth + ["-cv-covariance"], base + cvf + ["-cv-covariance"], base + ["-cv-covariance"],
                base + ["-live", "0", "-cv-covariance"], base + ["-live", "0"] + cvf + ["-cv-covariance"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-cv-covariance" in run.stdout and "smooth-covariance: " not in run.stdout, run.stdout
        assert not os.path.exists(os.path.join(folder, "final.smooth_covariance.yaml"))
