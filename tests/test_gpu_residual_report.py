"""aar_problem_residual_report on the device: per-detection errors against aar_eval_residuals, the exact lower median and maximum, the keep
flags of outlier rules, per-entity statistics against a numpy group-by, sharded problems, outlier recovery on contaminated data, the
aar_find_solution switches, and the cost of one call."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import aar
from aar import Problem
from conftest import load_golden
from pose_metrics import pose_delta_max

pytestmark = pytest.mark.gpu

CONVERGE = dict(max_iters=200, min_average_step_error_diff=0.0, min_step_error_diff=0.0, min_error=0.0)


def _ref_errors(p, x):
    r, _ = p.eval_residuals(x)
    r = r.reshape(-1, 8)
    return np.sqrt((r ** 2).sum(1) / 4), (r ** 2).sum(1)


def _x(p, ds, intrinsics):
    return p.x_with_intrinsics(ds.x_full) if intrinsics else ds.x_full


CASES = [("g1_cfg2", False), ("g2_small", False), ("g1_cfg3_cut", False), ("g1_cfg2_intr", True), ("cfg3", False)]


def _load(name):
    return aar.synth(3) if name == "cfg3" else load_golden(name)[0]


@pytest.mark.parametrize("name,intr", CASES)
@pytest.mark.parametrize("mode", [aar.RES_F32, aar.RES_F64])
def test_detection_errors_match_eval_residuals(name, intr, mode):
    ds = _load(name)
    with Problem(ds, residual_mode=mode, intrinsics=intr) as p:
        x = _x(p, ds, intr)
        e_ref, _ = _ref_errors(p, x)
        rr = p.residual_report(x)
    np.testing.assert_allclose(rr.det_err, e_ref, rtol=1e-15, atol=0)
    assert rr.keep.all() and rr.report["num_detections"] == ds.num_obs and rr.report["threshold"] == np.inf
    # Huber is ignored: the weighted problem reports the same bits as its plain twin
    with Problem(ds, residual_mode=mode, intrinsics=intr, with_huber=True) as p:
        rh = p.residual_report(x)
    assert np.array_equal(rh.det_err, rr.det_err)
    assert np.array_equal(rh.cam_stats, rr.cam_stats) and rh.report == rr.report


def _check_rule(rr, e, k_median, min_px, has_rule=True):
    n = len(e)
    med = np.sort(e)[(n - 1) // 2]
    rep = rr.report
    assert rep["median"] == med or (np.isnan(med) and np.isnan(rep["median"]))
    if has_rule and (k_median > 0 or min_px > 0):
        t = min_px if k_median <= 0 else max(min_px, k_median * med)
    else:
        t = np.inf
    assert rep["threshold"] == t
    assert np.array_equal(rr.keep, e <= t)
    assert rep["num_rejected"] == int((~(e <= t)).sum())
    return t


def test_order_statistics_and_keep_flags():
    ds = aar.synth(3)
    with Problem(ds) as p:
        x, _ = p.lm_solve(ds.x_full)
        rr0 = p.residual_report(x)
        e = rr0.det_err
        assert rr0.report["median"] == np.sort(e)[(len(e) - 1) // 2]
        assert rr0.report["max"] == e.max()
        for k_median, min_px in ((0, 0), (3, 0), (2, 0.5), (0, 0.4), (1, 0), (1, 100.0), (0.5, 0.1)):
            rr = p.residual_report(x, k_median, min_px)
            assert np.array_equal(rr.det_err, e)
            t = _check_rule(rr, e, k_median, min_px)
            print("rule (%g, %g): threshold %.6f px, %d rejected" % (k_median, min_px, t, rr.report["num_rejected"]))
        rn = p.residual_report(x, rule=False)   # NULL rule
        _check_rule(rn, e, 0, 0, has_rule=False)
        # a rule on a non-finite median is rejected as an invalid argument, not run
        with pytest.raises(aar.AarError) as err:
            p.residual_report(x, float("nan"), 0)
        assert err.value.code == aar.AAR_ERR_INVALID


def test_nan_frame_pose():
    ds, _ = load_golden("g1_cfg2")
    f = 7
    x = ds.x_full.copy()
    fr0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    x[fr0 + 6 * f:fr0 + 6 * f + 6] = np.nan
    bad = ds.obs_frame == f
    with Problem(ds) as p:
        rr = p.residual_report(x, 3, 0)
        rn = p.residual_report(x, rule=False)
    e = rr.det_err
    assert np.isnan(e[bad]).all() and np.isfinite(e[~bad]).all()
    assert rr.report["num_nonfinite"] == bad.sum() > 0
    assert np.isnan(rr.report["max"])
    _check_rule(rr, e, 3, 0)
    assert not rr.keep[bad].any()
    _check_rule(rn, e, 0, 0, has_rule=False)   # e <= +inf: NaN is dropped even without a rule
    assert rr.report["frames_emptied"] == 1
    assert np.isnan(rr.frame_stats[f, 1]) and rr.frame_stats[f, 3] == bad.sum()


def _groupby(idx, n, e, ss, keep):
    out = np.zeros((n, 4))
    for i in range(n):
        s = idx == i
        if s.any():
            out[i] = (s.sum(), ss[s].sum(), np.max(e[s]), (~keep[s]).sum())
    return out


def _check_stats(ds, rr, ss):
    e = rr.det_err
    for st, idx, n in ((rr.cam_stats, ds.obs_cam, ds.num_cams), (rr.marker_stats, ds.obs_marker, ds.num_markers),
                       (rr.frame_stats, ds.obs_frame, ds.num_frames)):
        want = _groupby(idx, n, e, ss, rr.keep)
        np.testing.assert_array_equal(st[:, [0, 2, 3]], want[:, [0, 2, 3]])
        np.testing.assert_allclose(st[:, 1], want[:, 1], rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", ["g1_cfg2", "g1_cfg3_cut", "cfg3"])
def test_entity_statistics_and_determinism(name):
    ds = _load(name)
    if name == "g1_cfg2":   # an unobserved marker and an empty frame get {0, 0, 0, 0}
        keep = (ds.obs_marker != 2) & (ds.obs_frame != 5)
        ds = ds.select_observations(keep)
    runs = {}
    for det in (False, True):
        with Problem(ds, deterministic=det) as p:
            _, ss = _ref_errors(p, ds.x_full)
            a = p.residual_report(ds.x_full, 2, 0)
            b = p.residual_report(ds.x_full, 2, 0)
        _check_stats(ds, a, ss)
        for k in ("det_err", "keep", "cam_stats", "marker_stats", "frame_stats"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.report == b.report
        runs[det] = a
    for k in ("det_err", "keep", "cam_stats", "marker_stats", "frame_stats"):
        assert np.array_equal(getattr(runs[False], k), getattr(runs[True], k)), k
    r = runs[False].report
    np.testing.assert_allclose(r["sum_sq"], runs[False].cam_stats[:, 1].sum(), rtol=1e-13)
    np.testing.assert_allclose(r["rmse"], np.sqrt(r["sum_sq"] / (4 * ds.num_obs)), rtol=1e-15)
    if name == "g1_cfg2":
        assert (runs[False].marker_stats[2] == 0).all() and (runs[False].frame_stats[5] == 0).all()


def _ranks(world, ds, x, k_median):
    group = aar.LocalGroup(world)
    out = [None] * world

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with Problem(ds, comm=comm) as p:
                out[r] = p.residual_report(x, k_median, 0)
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


@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank(world):
    ds = aar.synth(3)
    with Problem(ds) as p:
        one = p.residual_report(ds.x_full, 2.5, 0)
    out = _ranks(world, ds, ds.x_full, 2.5)
    assert np.array_equal(np.concatenate([o.keep for o in out]), one.keep)
    assert np.array_equal(np.concatenate([o.det_err for o in out]), one.det_err)
    filled = np.zeros(ds.num_frames, dtype=int)
    for o in out:
        for k in ("median", "max", "threshold", "num_detections", "num_rejected", "num_nonfinite", "cams_emptied", "markers_emptied",
                  "frames_emptied"):
            assert o.report[k] == one.report[k], k
        np.testing.assert_allclose(o.report["sum_sq"], one.report["sum_sq"], rtol=1e-12)
        for k in ("cam_stats", "marker_stats"):
            assert np.array_equal(getattr(o, k), getattr(out[0], k))   # the same bits on every rank
            np.testing.assert_allclose(getattr(o, k), getattr(one, k), rtol=1e-12, atol=0)
        mine = ~np.isnan(o.frame_stats[:, 0])
        filled += mine
        assert np.array_equal(o.frame_stats[mine], one.frame_stats[mine])
    assert (filled == 1).all()


def _corrupt(ds, frac, rng):
    """shift all four corners by 8-25 px on half of the chosen detections, rotate the corner order on the other half"""
    bad = rng.choice(ds.num_obs, int(round(frac * ds.num_obs)), replace=False)
    uv = ds.obs_uv.reshape(-1, 8).copy()
    half = len(bad) // 2
    for o in bad[:half]:
        a, r = rng.uniform(0, 2 * np.pi), rng.uniform(8, 25)
        uv[o] += np.tile([r * np.cos(a), r * np.sin(a)], 4).astype(np.float32)
    for o in bad[half:]:
        uv[o] = np.roll(uv[o].reshape(4, 2), 1, axis=0).reshape(-1)
    out = ds.select_observations(np.ones(ds.num_obs, dtype=bool))
    out.obs_uv = uv.reshape(ds.obs_uv.shape)
    return out, np.sort(bad)


def test_outlier_recovery():
    # Config 2 has 3-5 detections per frame: a corrupted detection drags its frame pose (and through the shared poses its neighbours) in
    # the contaminated least-squares solve, and clean detections there exceed 3 x median as well -- one rule applied to that solve empties
    # some frames (5 % of the detections go here).  What must hold: every corrupted detection goes, and the solution of what is left is
    # the clean one.
    clean = aar.synth(2)
    prm = aar.lm_default_params(**CONVERGE)
    ds, bad = _corrupt(clean, 0.02, np.random.default_rng(11))
    with Problem(ds, solver="direct") as p:
        x_c, _ = p.lm_solve(ds.x_full, params=prm)
        s2_before = p.covariance(x_c, frames=False).sigma2
        rr = p.residual_report(x_c, 3, 0)
    rejected = ~rr.keep
    is_bad = np.zeros(ds.num_obs, dtype=bool)
    is_bad[bad] = True
    print("median %.4f px, threshold %.4f px: %d rejected, %d of %d corrupted, %d clean (%d frames emptied); sigma2 before %.4f"
          % (rr.report["median"], rr.report["threshold"], rejected.sum(), (rejected & is_bad).sum(), len(bad), (rejected & ~is_bad).sum(),
             rr.report["frames_emptied"], s2_before))
    assert (rejected & is_bad).sum() == len(bad)          # every corrupted detection is rejected
    assert (rejected & ~is_bad).sum() <= 0.1 * ds.num_obs
    assert s2_before > 0.18
    ref_ds = clean.select_observations(rr.keep)
    filt = ds.select_observations(rr.keep)
    with Problem(ref_ds, solver="direct") as p:
        x_ref, _ = p.lm_solve(clean.x_full, params=prm)
    with Problem(filt, solver="direct") as p:
        x_f, _ = p.lm_solve(x_c, params=prm)
        s2_after = p.covariance(x_f, frames=False).sigma2
    # an emptied frame has no detection left: its pose stays wherever each solve started
    fr0 = 6 * (clean.num_cams - 1) + 6 * (clean.num_markers - 1)
    x_cmp = x_f.copy()
    for f in np.flatnonzero(np.bincount(filt.obs_frame, minlength=clean.num_frames) == 0):
        x_cmp[fr0 + 6 * f:fr0 + 6 * f + 6] = x_ref[fr0 + 6 * f:fr0 + 6 * f + 6]
    dr, dt = pose_delta_max(clean, x_ref, x_cmp)
    print("filtered vs reference solve: %.2e (rotation entries), %.2e m; sigma2 after %.4f" % (dr, dt, s2_after))
    # (the two solves start apart -- the filtered one where the contaminated solve ended -- and frames left with one or two detections are
    #  weakly determined: measured 5e-5 / 1e-5 m)
    assert dr < 1e-4 and dt < 1e-4
    assert abs(s2_after / 0.09 - 1) < 0.15


def test_find_solution_reject_outliers_switch(tmp_path):
    from conftest import PKG
    from test_residual_report_host import parse_residual_yaml
    exe = os.path.join(PKG, "aar_find_solution")
    got = {}
    for flag in ([], ["-reject-outliers", "3", "-covariance"]):
        folder = str(tmp_path / ("rej" if flag else "plain"))
        assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
        init = os.path.join(folder, "initial.solution")
        ds = aar.solution_read(init)
        bad_ds, bad = _corrupt(ds, 0.02, np.random.default_rng(5))
        aar.solution_write(init, bad_ds)
        run = subprocess.run([exe, folder, "0.05", "x", "-from-initial", "-solver", "direct"] + flag, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        res = os.path.join(folder, "final.residuals.yaml")
        assert os.path.exists(res) == bool(flag)
        assert os.path.exists(os.path.join(folder, "final.covariance.yaml")) == bool(flag)
        fin = aar.solution_read(os.path.join(folder, "final.solution"))
        assert np.array_equal(aar.solution_read(init).obs_uv, bad_ds.obs_uv)   # initial.solution is untouched
        got[bool(flag)] = fin.num_obs
        if not flag:
            assert fin.num_obs == ds.num_obs
            continue
        assert "outlier round 1" in run.stdout
        y = parse_residual_yaml(res)
        listed = set(t[:3] for t in y["rejected_detections"])
        injected = set((int(ds.frame_ids[ds.obs_frame[o]]), int(ds.cam_ids[ds.obs_cam[o]]), int(ds.marker_ids[ds.obs_marker[o]])) for o in bad)
        assert injected <= listed
        assert fin.num_obs == ds.num_obs - len(listed) == ds.num_obs - y["num_rejected"]
        assert y["num_detections"] == fin.num_obs
    assert got[True] < got[False]


def test_find_solution_residuals_switch_leaves_outputs_alone(tmp_path):
    from conftest import PKG
    from test_residual_report_host import parse_residual_yaml
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    env = dict(os.environ, AAR_DETERMINISTIC="1")
    got = {}
    for flag in ([], ["-residuals"]):
        run = subprocess.run([exe, folder, "0.05", "x", "-from-initial", "-solver", "direct"] + flag, capture_output=True, text=True, timeout=300, env=env)
        assert run.returncode == 0, run.stderr
        assert os.path.exists(os.path.join(folder, "final.residuals.yaml")) == bool(flag)
        got[bool(flag)] = [open(os.path.join(folder, f), "rb").read() for f in ("final.solution", "final.solution.yaml")]
    assert got[False] == got[True]
    y = parse_residual_yaml(os.path.join(folder, "final.residuals.yaml"))
    assert y["num_rejected"] == 0 and y["rejected_detections"] == [] and y["threshold"] == np.inf


def _time_call(p, x, reps=10):
    """wall time of one aar_problem_residual_report without the per-detection host copies (entity and frame stats still come back)"""
    ds = p.ds
    cs, ms, fs = np.zeros((ds.num_cams, 4)), np.zeros((ds.num_markers, 4)), np.zeros((ds.num_frames, 4))
    rule = aar.COutlierRule()
    rule.struct_size, rule.k_median, rule.min_px = C.sizeof(rule), 3.0, 0.0
    rep = aar.CResidualReport()
    rep.struct_size = C.sizeof(rep)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    L = aar.lib()
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        assert L.aar_problem_residual_report(p.handle, dp(x), C.byref(rule), None, None, dp(cs), dp(ms), dp(fs), C.byref(rep)) == 0
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:])), rep


@pytest.mark.parametrize("cfg", [3, 5])
def test_cost_full_size(cfg):
    ds = aar.synth(cfg)
    with Problem(ds) as p:
        x = ds.x_full
        dt, rep = _time_call(p, x)
        rr = p.residual_report(x, 3, 0)
    assert rep.num_detections == ds.num_obs and rep.median == rr.report["median"]
    e = rr.det_err
    assert rr.report["median"] == np.sort(e)[(len(e) - 1) // 2] and rr.report["max"] == e.max()
    print("config %d: %d detections, one residual report %.3f ms (median of 10, no per-detection copies)" % (cfg, ds.num_obs, dt * 1e3))
