"""Pose covariance of smoothed tracks (aar_track_smooth_covariance): the diagonal and lag-one blocks of H^-1 from the
device's downward pass over the cyclic reduction's elimination tree.  Needs a real MI355X.

Yardstick: numpy.linalg.inv of the dense H built from the blocks aar_track_smooth_system returned at mu = 0 (the assembly is certified by
tests/test_gpu_track_smooth.py), itself checked by long-double iterative refinement of its columns.
Bar (frame_cov and lag_cov alike): largest entry error over the largest entry of the yardstick's selected blocks <= 10 eps kappa_2(H), kappa_2
from numpy on the same H (the ratio of the extreme eigenvalues of the symmetric positive definite H).  That is the forward-error order of any
inverse, not a measured figure.  Above 500 frames, where the dense inverse is out of reach, columns of the inverse from
smooth_restated.solve on unit right-hand sides take its place, with kappa_2 from scipy.linalg.eigvals_banded.
Block rows: (H Sigma)_ff = I and the two off-diagonal positions the selected blocks determine, normalised by sum_j |H_fj| |Sigma_jf|, held to
100 x NUMPY_BLOCK_ROW = the largest value numpy's own inverse reaches on the cases of up to 500 frames.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.linalg import eigvals_banded

import aar
import smooth_cases as sc
import smooth_covariance_restated as scr
import smooth_restated as sr
import track_restated as tr
from conftest import PKG, ROOT
from test_gpu_live_marginal import parse_live_cov_yaml
from test_gpu_track_smooth import SROT, STRANS, _gaps, _golden_track, _problem, _shape_dataset, _system_inputs

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# the largest block-row residual of numpy.linalg.inv itself over the shapes of up to 500 frames below (on the restated systems of the same
# inputs, measured on the CPU; DESIGN.md section 28 has the table)
NUMPY_BLOCK_ROW = 1.84e-13


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _kappa(H):
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    return float(ev[-1] / ev[0])


def _times(diag, off, X):
    """H X for X [F, 6, n] from the blocks, in X's precision"""
    Y = np.einsum("fij,fjn->fin", diag.astype(X.dtype), X)
    if diag.shape[0] > 1:
        o = off.astype(X.dtype)
        Y[:-1] += np.einsum("fij,fjn->fin", o, X[1:])
        Y[1:] += np.einsum("fji,fjn->fin", o, X[:-1])
    return Y


def _refined(H, diag, off, X0):
    """long-double iterative refinement of the columns X0 [6F, n] of an inverse: residual in long double, correction by numpy's solve"""
    F = diag.shape[0]
    n = X0.shape[1]
    X = X0.astype(np.longdouble)
    assert n == 6 * F
    I = np.eye(n, dtype=np.longdouble)
    for _ in range(3):
        r = (I - _times(diag, off, X.reshape(F, 6, n)).reshape(6 * F, n)).astype(np.float64)
        X = X + np.linalg.solve(H, r)
    return X


def _errors(S, R, Sd, Rd):
    e_s = float(np.abs(S - Sd).max() / np.abs(Sd).max())
    e_r = float(np.abs(R - Rd).max() / np.abs(Rd).max()) if len(Rd) else 0.0
    return e_s, e_r


def _against_the_inverse(tag, gd, go, S, R, refine=True):
    """the comparison of section 1; returns (kappa, numpy's own block-row residual)"""
    F = gd.shape[0]
    H = sr.dense(gd, go)
    Hi = np.linalg.inv(H)
    kappa = _kappa(H)
    bar = 10 * EPS * kappa
    if refine:
        X = _refined(H, gd, go, Hi)
        e_y = float(np.abs(Hi - X).max() / np.abs(X).max())
        assert e_y <= bar, ("the yardstick itself", e_y, bar)
    else:
        e_y = float("nan")
    Sd, Rd = scr.selected_blocks(Hi, F)
    e_s, e_r = _errors(S, R, Sd, Rd)
    rows_np = scr.block_row_residual(gd, go, Sd, Rd)
    print("%s: kappa %.3e, yardstick %.2e, frame_cov %.2e lag_cov %.2e = %.4f / %.4f eps kappa; block rows: numpy %.2e" %
          (tag, kappa, e_y, e_s, e_r, e_s / (EPS * kappa), e_r / (EPS * kappa), rows_np))
    assert e_s <= bar and e_r <= bar, (e_s, e_r, bar)
    return kappa, rows_np


# ---- 1. blocks against the inverse ----
@pytest.mark.parametrize("variant", ["plain", "gaps", "rel", "gaps_rel"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_blocks_against_the_inverse(which, variant):
    name, ds, x0, delta = _system_inputs()[which]
    F = ds.num_frames
    ft = _gaps(F) if "gaps" in variant else None
    rng = np.random.default_rng(3)
    rel = rng.normal(size=(F - 1, 6)) * [0.05, 0.05, 0.05, 0.02, 0.02, 0.02] if "rel" in variant else None
    with _problem(ds, delta) as p:
        gd, go, _, _, cost = p.track_smooth_system(x0, SROT, STRANS, 0.0, frame_time=ft, rel_motion=rel)
        S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS, frame_time=ft, rel_motion=rel)
    assert S.shape == (F, 6, 6) and R.shape == (F - 1, 6, 6)
    _against_the_inverse("%s %s" % (name, variant), gd, go, S, R)
    rows = scr.block_row_residual(gd, go, S, R)
    print("    block rows: device %.2e" % rows)
    assert rows <= 100 * NUMPY_BLOCK_ROW, rows
    assert rep["num_residuals"] == 8 * ds.num_obs + 6 * (F - 1) and rep["num_vars"] == 6 * F
    assert (rep["data_cost"], rep["prior_cost"]) == cost
    np.testing.assert_allclose(rep["sigma2"], (cost[0] + cost[1]) / (rep["num_residuals"] - rep["num_vars"]), rtol=1e-15)
    assert rep["launches"] == 2 + 1 + 1 and rep["seconds"] > 0


# ---- 2. every launch shape ----
def _column_frames(F):
    """about ten frames for the column check: the ends, an emptied one, both sides of the launch boundaries (tail / separate level, the
    64-thread groups of a separate level, the top strides)"""
    s0 = 1
    while s0 < F and (F + 2 * s0 - 1) // (2 * s0) > 256:
        s0 *= 2
    pick = [0, 1, F - 2, F - 1, F // 3 + 5, 127, 128, 129, s0, s0 + 1, 2 * s0 * 255 + s0, 512, 1024]
    return sorted(set(f for f in pick if 0 <= f < F))


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 63, 64, 65, 127, 500, 513, 1100, 2000])
def test_every_launch_shape(F):
    ds = _shape_dataset(F)
    assert ds.num_frames == F
    x0 = sc.track_start(ds)
    ft = _gaps(F) if F > 1 else None
    with aar.Problem(ds) as p:
        gd, go, _, _, _ = p.track_smooth_system(x0, SROT, STRANS, 0.0, frame_time=ft)
        S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS, frame_time=ft)
    levels = 0
    s = 1
    while s < F and (F + 2 * s - 1) // (2 * s) > 256:
        s *= 2
        levels += 1
    assert levels == (0 if F <= 512 else 1 if F <= 1024 else 2)
    assert rep["launches"] == 2 + (1 + 2 * levels + (1 if levels else 0)) + (1 + levels)
    if F <= 500:
        _against_the_inverse("F %d" % F, gd, go, S, R, refine=F <= 127)
    else:
        ab = sr.banded(gd, go)
        n = 6 * F
        lo = eigvals_banded(ab, lower=True, select="i", select_range=(0, 0))[0]
        hi = eigvals_banded(ab, lower=True, select="i", select_range=(n - 1, n - 1))[0]
        assert lo > 0
        kappa = float(hi / lo)
        frames = _column_frames(F)
        E = np.zeros((n, 6 * len(frames)))
        for k, f in enumerate(frames):
            E[6 * f:6 * f + 6, 6 * k:6 * k + 6] = np.eye(6)
        X = sr.solve(gd, go, E, 0.0)
        big, err = 0.0, 0.0
        for k, f in enumerate(frames):
            col = X[:, 6 * k:6 * k + 6]
            want = [(S[f], col[6 * f:6 * f + 6])]
            if f + 1 < F:
                want.append((R[f], col[6 * f + 6:6 * f + 12].T))      # Sigma_{f+1,f} = Sigma_{f,f+1}^T
            if f > 0:
                want.append((R[f - 1], col[6 * f - 6:6 * f]))         # Sigma_{f-1,f}
            for got, ref in want:
                big = max(big, float(np.abs(ref).max()))
                err = max(err, float(np.abs(got - ref).max()))
        print("F %d: kappa %.3e, %d frames' columns: %.2e = %.4f eps kappa" % (F, kappa, len(frames), err / big, err / big / (EPS * kappa)))
        assert err / big <= 10 * EPS * kappa, (err / big, 10 * EPS * kappa)
    rows = scr.block_row_residual(gd, go, S, R)
    print("F %d: block rows: device %.2e (launches %d)" % (F, rows, rep["launches"]))
    assert rows <= 100 * NUMPY_BLOCK_ROW, rows
    assert np.array_equal(S, np.swapaxes(S, 1, 2))


# ---- 3. properties ----
def test_properties():
    F = 65
    ds = _shape_dataset(F)
    x0 = sc.track_start(ds)
    ft = _gaps(F)
    keep = np.array(x0)
    with aar.Problem(ds) as p:
        a0 = p.track_smooth(x0, SROT, STRANS, frame_time=ft)
        S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS, frame_time=ft)
        S2, R2, rep2 = p.track_smooth_covariance(x0, SROT, STRANS, frame_time=ft)
        a1 = p.track_smooth(x0, SROT, STRANS, frame_time=ft)
    with aar.Problem(ds) as p:
        b = p.track_smooth(x0, SROT, STRANS, frame_time=ft)
    assert np.array_equal(x0, keep)                                   # x_full is not modified
    assert np.array_equal(S, S2) and np.array_equal(R, R2)            # two calls give identical bits
    for k in ("num_residuals", "num_vars", "data_cost", "prior_cost", "sigma2", "launches"):
        assert rep[k] == rep2[k], k
    for u, v, w in zip(a0, a1, b):                                    # aar_track_smooth before and after: the bits of a problem never asked
        if isinstance(u, dict):
            for k in u:
                assert k == "seconds" or u[k] == v[k] == w[k], k
        else:
            assert np.array_equal(u, v) and np.array_equal(u, w)
    assert np.array_equal(S, np.swapaxes(S, 1, 2))                    # the kernel mirrors the lower triangle: symmetric to the bit
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(R))
    assert min(np.linalg.eigvalsh(S[f])[0] for f in range(F)) > 0
    rel = [S[f] + S[f + 1] - R[f] - R[f].T for f in range(F - 1)]      # Cov(z_{f+1} - z_f), up to sigma2
    assert min(np.linalg.eigvalsh(0.5 * (m + m.T))[0] for m in rel) > 0
    # a frame without detections is carried by its neighbours: finite, and less certain than the observed frames on either side of its run
    empty = sc.emptied(F)
    cnt = np.bincount(ds.obs_frame, minlength=F)
    assert np.all(cnt[empty] == 0)
    tvar = np.einsum("fii->f", S[:, 3:, 3:])
    run = [f for f in empty if 0 < f < F - 1]
    left, right = run[0] - 1, run[-1] + 1
    assert cnt[left] > 0 and cnt[right] > 0 and cnt[1] > 0 and cnt[F - 2] > 0
    for f in run:
        assert tvar[f] > tvar[left] and tvar[f] > tvar[right], f
    assert tvar[0] > tvar[1] and tvar[F - 1] > tvar[F - 2]
    print("translation variance (unscaled): observed neighbours %.3e %.3e, emptied run %s" % (tvar[left], tvar[right], np.array2string(tvar[run], precision=3)))


# ---- 4. consistency with the estimator ----
def test_consistency_with_the_estimator():
    ds, x0, zt = sc.static_object(64)
    F = ds.num_frames
    n0 = sc.ns(ds)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, srep, _, _ = p.track_smooth(xt, SROT, STRANS)
        S, R, rep = p.track_smooth_covariance(xs, SROT, STRANS)
    td = tr.TrackData(ds, xt)
    sp = sr.SmoothProblem(td, SROT, STRANS)
    r = sr.smooth_lm(sp, td.z0)
    assert r["margin"] > 1e-9 and srep["iterations"] == r["iterations"]
    diag, off, _ = sp.system(r["z"])
    H = sr.dense(diag, off)
    kappa = _kappa(H)
    Sd, Rd = scr.selected_blocks(np.linalg.inv(H), F)
    rows = 8 * ds.num_obs + 6 * (F - 1)
    sigma2 = r["err"] / (rows - 6 * F)
    e_s, e_r = _errors(S, R, Sd, Rd)
    e_2 = abs(rep["sigma2"] - sigma2) / sigma2
    print("static object: kappa %.3e, sigma2 %.6e (restated %.6e, %.2e), frame_cov %.2e lag_cov %.2e = %.4f / %.4f eps kappa" %
          (kappa, rep["sigma2"], sigma2, e_2, e_s, e_r, e_s / (EPS * kappa), e_r / (EPS * kappa)))
    bar = 10 * EPS * kappa
    assert e_2 <= bar and e_s <= bar and e_r <= bar, (e_2, e_s, e_r, bar)

    def mahalanobis(z, s2, blocks):
        d = z.reshape(F, 6) - zt
        return float(np.mean([d[f] @ np.linalg.solve(s2 * blocks[f], d[f]) for f in range(F)]))
    m_dev = mahalanobis(xs[n0:n0 + 6 * F], rep["sigma2"], S)
    m_ref = mahalanobis(r["z"], sigma2, Sd)
    print("static object: mean squared Mahalanobis distance to the truth %.6f (restated %.6f); 6 would be a calibrated, independent estimate" % (m_dev, m_ref))
    assert abs(m_dev - m_ref) <= 1e-6 * m_ref, (m_dev, m_ref)


# ---- 5. edges and interfaces ----
def _raw(p, x0, F, frame_cov=True, lag_cov=True, report=True, struct_size=None, fill=7.0):
    """the C call with sentinel-filled outputs: (code, frame_cov, lag_cov, report struct)"""
    x = np.array(p._x(x0), dtype=np.float64)
    keep = x.copy()
    spar = aar.SmoothParams(SROT, STRANS)
    fc, lc = np.full((max(F, 1), 6, 6), fill), np.full((max(F - 1, 1), 6, 6), fill)
    rep = aar.CSmoothCovarianceReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep) if struct_size is None else struct_size
    code = aar.lib().aar_track_smooth_covariance(p.handle, aar._dptr(x), C.byref(spar.c), aar._dptr(fc) if frame_cov else None,
                                                 aar._dptr(lc) if lag_cov else None, C.byref(rep) if report else None)
    assert np.array_equal(x, keep)
    return code, fc, lc, rep


def test_no_detection_anywhere_is_a_numeric_error():
    ds = sc.without_frames(aar.synth(2, num_frames=6), range(6))
    assert ds.num_obs == 0
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        code, fc, lc, rep = _raw(p, x0, 6)
        assert code == aar.AAR_ERR_NUMERIC
        assert np.all(fc == 7.0) and np.all(lc == 7.0)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_covariance(x0, SROT, STRANS)
        assert e.value.code == aar.AAR_ERR_NUMERIC
    one = sc.without_frames(aar.synth(2, num_frames=1), [0])          # F = 1 and nothing seen
    with aar.Problem(one) as p:
        code, fc, lc, rep = _raw(p, sc.track_start(one), 1)
        assert code == aar.AAR_ERR_NUMERIC and np.all(fc == 7.0)


def test_one_frame_is_the_inverse_of_its_block():
    one = aar.synth(2, num_frames=1)
    x0 = sc.track_start(one)
    with aar.Problem(one) as p:
        gd, go, _, _, cost = p.track_smooth_system(x0, SROT, STRANS, 0.0)
        S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS)
    assert S.shape == (1, 6, 6) and R.shape == (0, 6, 6) and rep["launches"] == 4
    V = gd[0]
    kappa = _kappa(V)
    Vi = np.linalg.inv(V)
    assert np.abs(S[0] - Vi).max() / np.abs(Vi).max() <= 10 * EPS * kappa
    assert rep["num_residuals"] == 8 * one.num_obs and rep["num_vars"] == 6 and rep["prior_cost"] == 0.0
    np.testing.assert_allclose(rep["sigma2"], cost[0] / (8 * one.num_obs - 6), rtol=1e-15)


def test_null_outputs_and_truncated_report():
    ds, _ = _golden_track("g_track_cfg2")
    x0, F = ds.x_full, ds.num_frames
    with aar.Problem(ds) as p:
        code, fc, lc, rep = _raw(p, x0, F)
        assert code == 0 and not np.any(fc == 7.0) and not np.any(lc == 7.0)
        for kw in (dict(frame_cov=False), dict(lag_cov=False), dict(report=False), dict(frame_cov=False, lag_cov=False, report=False)):
            code, fc2, lc2, rep2 = _raw(p, x0, F, **kw)
            assert code == 0, kw
            assert np.array_equal(fc2, fc) if kw.get("frame_cov", True) else np.all(fc2 == 7.0)
            assert np.array_equal(lc2, lc) if kw.get("lag_cov", True) else np.all(lc2 == 7.0)
            if kw.get("report", True):
                assert rep2.sigma2 == rep.sigma2 and rep2.num_vars == 6 * F
        # a caller compiled against a shorter report: the fields beyond its struct_size are not written
        cut = aar.CSmoothCovarianceReport.data_cost.offset
        code, _, _, rep3 = _raw(p, x0, F, struct_size=cut)
        assert code == 0 and rep3.struct_size == cut and rep3.num_residuals == rep.num_residuals and rep3.num_vars == rep.num_vars
        untouched = bytes(bytearray(rep3)[cut:])
        assert untouched == b"\x55" * (C.sizeof(rep3) - cut)
        # invalid parameters are refused by aar_smooth_params_validate
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_covariance(x0, -1.0, STRANS)
        assert e.value.code == aar.AAR_ERR_INVALID


def test_unsupported_behind_a_communicator():
    ds, _ = _golden_track("g_track_cfg2")
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            with pytest.raises(aar.AarError) as e:
                p.track_smooth_covariance(ds.x_full, SROT, STRANS)
            assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    finally:
        comm.close()
        group.close()


def test_huber_problem():
    ds, _ = _golden_track("g_track_cfg2_huber")
    x0 = ds.x_full
    out = {}
    for delta in (None, 1.0):
        with _problem(ds, delta) as p:
            gd, go, _, _, _ = p.track_smooth_system(x0, SROT, STRANS, 0.0)
            S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS)
        _against_the_inverse("huber delta %s" % delta, gd, go, S, R)
        out[delta] = (S, rep)
    # the Huber weights are in H and in the cost: down-weighted detections leave the poses less certain
    assert out[1.0][1]["data_cost"] < out[None][1]["data_cost"]
    assert np.einsum("fii->", out[1.0][0]) > np.einsum("fii->", out[None][0])


def test_intrinsics_problem():
    ds, _ = _golden_track("g_track_cfg2")
    F = ds.num_frames
    with aar.Problem(ds, intrinsics=True) as p:
        x0 = p.x_with_intrinsics(ds.x_full)
        n0 = sc.ns(ds)
        q = x0[n0 + 6 * F:].reshape(ds.num_cams, 9)
        q[:, 0] *= 1.01
        q[:, 1] += 3.0
        gd, go, _, _, _ = p.track_smooth_system(x0, SROT, STRANS, 0.0)
        S, R, rep = p.track_smooth_covariance(x0, SROT, STRANS)
    with aar.Problem(ds) as p:
        S0, _, _ = p.track_smooth_covariance(ds.x_full, SROT, STRANS)
    _against_the_inverse("intrinsics", gd, go, S, R)
    assert np.abs(S - S0).max() > 1e-3 * np.abs(S0).max()           # the K of the pose vector is the one used
    assert rep["num_vars"] == 6 * F


def _kv(stdout):
    return dict(l.split(" = ") for l in stdout.splitlines() if " = " in l)


def test_mapper_track_smooth_covariance(tmp_path):
    exe = str(tmp_path / "smooth_covariance_mapper_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_covariance_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                         "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = _kv(run.stdout)
    ds = aar.synth(2)
    F = ds.num_frames
    x0 = sc.track_start(ds)
    ft = np.asarray(ds.frame_ids, dtype=np.float64)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, _, _, _ = p.track_smooth(xt, SROT, STRANS, frame_time=ft)
        S, R, rep = p.track_smooth_covariance(xs, SROT, STRANS, frame_time=ft)
    assert int(kv["frames"]) == F and int(kv["pairs"]) == F - 1
    assert int(kv["num_residuals"]) == rep["num_residuals"] and int(kv["num_vars"]) == rep["num_vars"] and int(kv["launches"]) == rep["launches"]
    # (the mapper carries its poses as 4x4 matrices between its calls: a few ulps of the point, 1e-8 in the poses as tests/test_gpu_track_smooth.py
    # holds them; the blocks follow the point)
    np.testing.assert_allclose(float(kv["sigma2"]), rep["sigma2"], rtol=1e-7)
    Sm = np.array([[float(v) for v in kv["S%d" % f].split()] for f in range(F)]).reshape(F, 6, 6)
    Rm = np.array([[float(v) for v in kv["R%d" % f].split()] for f in range(F - 1)]).reshape(F - 1, 6, 6)
    assert np.abs(Sm - S).max() <= 1e-6 * np.abs(S).max() and np.abs(Rm - R).max() <= 1e-6 * np.abs(R).max()


def test_find_solution_smooth_covariance_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # The blocks are over (rvec, t), and the solution file holds every pose after a vec -> matrix -> vec round trip.  Config 2's last frames turn
    # through pi (frame 98: 3.1409 rad), where that round trip lands on another rotation vector of the same rotation and the blocks read back
    # from the file would be in other coordinates than the driver's.  The recording is cut before them (the first 90 frames: below 2.95 rad).
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    run = subprocess.run(base + ["-smooth", repr(SROT), repr(STRANS), "-smooth-covariance"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, AAR_DETERMINISTIC="1"))
    assert run.returncode == 0, run.stdout + run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("smooth-covariance: ")]
    assert len(line) == 1 and "smooth: " in run.stdout, run.stdout
    y = parse_live_cov_yaml(os.path.join(folder, "final.smooth_covariance.yaml"))
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    F = got.num_frames
    assert F == FK and np.linalg.norm(got.x_full[n0:n0 + 6 * F].reshape(F, 6)[:, :3], axis=1).max() < 3.0
    with aar.Problem(got) as p:
        S, R, rep = p.track_smooth_covariance(got.x_full, SROT, STRANS, frame_time=np.asarray(got.frame_ids, dtype=np.float64))
    assert sorted(y) == sorted(int(i) for i in got.frame_ids)
    for f in range(F):
        sig, blk = y[int(got.frame_ids[f])]
        np.testing.assert_allclose(sig, rep["sigma2"], rtol=1e-6)
        assert np.abs(blk - rep["sigma2"] * S[f]).max() <= 1e-6 * np.abs(rep["sigma2"] * S[f]).max(), f
    words = line[0].replace(",", " ").split()
    s1 = np.sqrt(rep["sigma2"] * np.einsum("fii->f", S[:, 3:, 3:]))
    np.testing.assert_allclose(float(words[words.index("sigma2") + 1]), rep["sigma2"], rtol=1e-4)
    np.testing.assert_allclose([float(words[words.index("largest") + 1]), float(words[words.index("smallest") + 1])], [s1.max(), s1.min()], rtol=1e-4)
    # without -smooth-covariance no file is written; the flag without -smooth is refused with the usage message
    os.remove(os.path.join(folder, "final.smooth_covariance.yaml"))
    run = subprocess.run(base + ["-smooth", repr(SROT), repr(STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "smooth-covariance: " not in run.stdout and not os.path.exists(os.path.join(folder, "final.smooth_covariance.yaml"))
    for bad in (base + ["-smooth-covariance"], base + ["-live", "0", "-smooth-covariance"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-smooth-covariance" in run.stdout and "smooth-covariance: " not in run.stdout, run.stdout
