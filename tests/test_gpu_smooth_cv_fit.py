"""Fitting the constant-velocity smoother's noise levels (aar_track_smooth_fit2, aar_track_smooth_fit_terms2) against the float64
restatement tests/smooth_cv_fit_restated.py (numpy.linalg.inv of the dense H, the term's 6x18 Jacobian by complex step).  Needs a real MI355X.

Bars: the entries' terms, their sums and u_0 10 eps kappa_2(H) relative to the reference value (section 29's bar; section 32 holds the blocks the
terms are built from to it); the path of a fixed-length run 1e-8 relative with equal LM step counts; recovery within smooth_cv_fit_cases.CAPS.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_fit_cases as cc
import smooth_cv_fit_restated as cfr
import smooth_fit_cases as fc
import track_restated as tr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SROT, STRANS, SROT0, STRANS0, CV = cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0, cc.CV
SENT = -7.25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _kappa(H):
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    return float(ev[-1] / ev[0])


def _frames(ds, x):
    n0 = sc.ns(ds)
    return np.asarray(x)[n0:n0 + 6 * ds.num_frames].reshape(-1, 6)


# ---- 1. the terms, the sums and u_0 against the restatement, on the device's own track ----
def _check_terms(ds, x, ft, label, turned_at=None):
    F = ds.num_frames
    td = tr.TrackData(ds, x)
    e = cfr.estep(cfr.CvFitProblem(td, SROT0, STRANS0, ft), td.z0, SROT, STRANS, SROT0, STRANS0)
    kappa = _kappa(e["H"])
    bar = 10 * EPS * kappa
    with aar.Problem(ds) as p:
        terms, sums = p.track_smooth_fit_terms2(x, SROT, STRANS, frame_time=ft, **CV)
    assert terms.shape == (F - 1, 4) and sums.shape == (6,)
    if turned_at is not None:
        assert abs(np.sqrt(e["terms"][turned_at, 0] * np.diff(ft)[turned_at]) - 3.0) < 1e-6      # the 3 rad term is in
    want = np.r_[e["sums"], e["u_0"], e["pair0_cost"]]
    e_t = float(np.max(np.abs(terms - e["terms"]) / np.abs(e["terms"])))
    e_s = float(np.max(np.abs(sums - want) / np.abs(want)))
    print("%s: kappa %.3e, terms %.2e sums, u_0 and pair 0's cost %.2e = %.4f / %.4f eps kappa" % (label, kappa, e_t, e_s, e_t / (EPS * kappa),
                                                                                                   e_s / (EPS * kappa)))
    assert e_t <= bar and e_s <= bar, (e_t, e_s, bar)
    # the prior's share of tr(H H^-1) = 6 F lies strictly between nothing and all of it
    share = sums[1] / SROT ** 2 + sums[3] / STRANS ** 2 + sums[4]
    assert 0 < share < 6 * F, (share, 6 * F)
    assert np.all(terms[:, [1, 3]] > 0) and np.all(terms >= 0)


@pytest.mark.parametrize("F", [3, 4, 5, 65, 66, 67, 129, 258, 259, 515])
def test_terms_against_the_restatement(F):
    ds, x0, ft = cc.terms_case(F)
    with aar.Problem(ds) as p:
        x = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)[0]
    _check_terms(ds, x, ft, "F %d" % F)


def test_terms_with_a_residual_rotation_near_three_rad():
    F, k = 17, 8
    ds, x0, ft = cc.terms_case(F)
    _check_terms(ds, cc.turned(ds, x0, ft, k), ft, "F %d, term %d turned" % (F, k), turned_at=k)


# ---- 2. a fixed-length run against the restated loop ----
@functools.lru_cache(maxsize=None)
def _loop_case(name):
    if name == "plain48":
        ds, x0 = cc.cv_sequence(48, *cc.CV_SIGMAS, seed=5)
        return ds, x0, None
    ds = fc.shape_dataset(65)
    return ds, sc.track_start(ds), fc.gaps(65)


@pytest.mark.parametrize("name", ["plain48", "emptied65_gaps"])
def test_fixed_length_run_against_the_restated_loop(name):
    ds, x0, ft = _loop_case(name)
    td = tr.TrackData(ds, x0)
    r = cfr.fit(cfr.CvFitProblem(td, SROT0, STRANS0, ft), td.z0, SROT, STRANS, max_iters=5, rel_tol=0.0)
    print("%s: the restated runs' smallest decision margin %.2e" % (name, r["margin"]))
    assert r["margin"] > 1e-9 and r["iterations"] == 5 and r["stop_code"] == 2        # no LM decision of the restated runs is a toss-up
    with aar.Problem(ds) as p:
        x, rep, path = p.track_smooth_fit2(x0, SROT, STRANS, frame_time=ft, fit=dict(max_iters=5, rel_tol=0.0), **CV)
    assert rep["iterations"] == 5 and rep["stop_code"] == 2 and path.shape == (6, 3)
    err = float(np.max(np.abs(path - r["path"]) / r["path"]))
    print("%s: path %.2e, lm_steps %d (restated %d), sigmas %s" % (name, err, rep["lm_steps"], r["lm_steps"], np.array2string(path[-1], precision=6)))
    assert np.array_equal(path[0], [1.0, SROT, STRANS])
    assert err <= 1e-8, err
    assert rep["lm_steps"] == r["lm_steps"]
    assert (rep["sigma_px"], rep["sigma_rot"], rep["sigma_trans"]) == tuple(path[-1])
    np.testing.assert_allclose([rep["sigma_rot_eff"], rep["sigma_trans_eff"]], [path[-1, 1] / path[-1, 0], path[-1, 2] / path[-1, 0]], rtol=1e-15)
    np.testing.assert_allclose([rep["a_rot"], rep["u_rot"], rep["a_trans"], rep["u_trans"]], r["sums"], rtol=1e-7)
    np.testing.assert_allclose([rep["u_data"], rep["data_cost"]], [r["U_d"], r["data_cost"]], rtol=1e-7)
    n0 = sc.ns(ds)
    assert np.array_equal(x[:n0], x0[:n0]) and np.abs(_frames(ds, x) - r["z"]).max() < 1e-7
    assert rep["launches"] > 0 and rep["seconds"] > 0


# ---- 3. recovery, 4. fixed point, 5. two identical calls ----
@functools.lru_cache(maxsize=None)
def _device_fit(seed):
    ds, x0 = cc.cv_walk(seed)
    with aar.Problem(ds) as p:
        a = p.track_smooth_fit2(x0, SROT, STRANS, fit=dict(max_iters=cc.CV_MAX_ITERS), **CV)
        b = p.track_smooth_fit2(x0, SROT, STRANS, fit=dict(max_iters=cc.CV_MAX_ITERS), **CV)
        x, rep, _ = a
        eff = dict(model=1, sigma_rot0=SROT0 / rep["sigma_px"], sigma_trans0=STRANS0 / rep["sigma_px"])
        terms, sums = p.track_smooth_fit_terms2(x, rep["sigma_rot_eff"], rep["sigma_trans_eff"], **eff)
        cost = p.track_smooth_system2(x, rep["sigma_rot_eff"], rep["sigma_trans_eff"], 0.0, **eff)[5]
    return ds, a, b, sums, cost


def test_recovery_on_the_device():
    ds, (x, rep, path), _, _, _ = _device_fit(100)
    dev = np.array([rep["sigma_px"], rep["sigma_rot"], rep["sigma_trans"]]) / cc.CV_SIGMAS - 1.0
    print("seed 100: %d EM iterations (exit %d, %d LM steps, %d launches, %.3f s), deviations %s" %
          (rep["iterations"], rep["stop_code"], rep["lm_steps"], rep["launches"], rep["seconds"], np.array2string(dev, precision=5)))
    assert rep["stop_code"] == 1 and rep["iterations"] < cc.CV_MAX_ITERS and rep["last_rel_change"] < 1e-3
    assert np.all(np.abs(dev) <= cc.CAPS), (dev, cc.CAPS)


def test_fixed_point():
    ds, (x, rep, path), _, sums, cost = _device_fit(100)
    F, N = ds.num_frames, ds.num_obs
    q, s_r, s_t = rep["sigma_px"] ** 2, rep["sigma_rot"] ** 2, rep["sigma_trans"] ** 2
    U_d = 6.0 * F - sums[1] / rep["sigma_rot_eff"] ** 2 - sums[3] / rep["sigma_trans_eff"] ** 2 - sums[4]
    new = cfr.mstep(sums, cost[0], U_d, q, s_r, s_t, F, N)
    move = max(abs(np.sqrt(a) / np.sqrt(b) - 1.0) for a, b in zip(new, (q, s_r, s_t)))
    print("one more E-step and M-step at the reported values moves a sigma by at most %.2e" % move)
    assert move <= 1e-3, move


def test_two_identical_calls():
    _, (xa, ra, pa), (xb, rb, pb), _, _ = _device_fit(100)
    assert np.array_equal(xa, xb) and np.array_equal(pa, pb)
    for k in ra:
        assert k == "seconds" or ra[k] == rb[k], k


# ---- 6. held parameters ----
def test_held_parameters():
    ds, x0, ft = _loop_case("emptied65_gaps")
    with aar.Problem(ds) as p:
        x, rep, path = p.track_smooth_fit2(x0, SROT, STRANS, frame_time=ft, fit=dict(estimate_px=0, max_iters=8), **CV)
        y, rep2, path2 = p.track_smooth_fit2(x0, SROT, STRANS, frame_time=ft, fit=dict(estimate_px=0, estimate_trans=0, max_iters=8), **CV)
        w, rep3, path3 = p.track_smooth_fit2(x0, SROT, STRANS, frame_time=ft, fit=dict(estimate_rot=0, max_iters=8), **CV)
    assert rep["sigma_px"] == 1.0 and np.all(path[:, 0] == 1.0)
    assert rep["sigma_rot_eff"] == rep["sigma_rot"] and rep["sigma_trans_eff"] == rep["sigma_trans"]
    assert rep["sigma_rot"] != SROT and rep["sigma_trans"] != STRANS
    assert np.all(path2[:, 2] == STRANS) and rep2["sigma_px"] == 1.0 and rep2["sigma_rot"] != SROT   # a sigma held fixed stays at its start value
    assert np.all(path3[:, 1] == SROT) and rep3["sigma_px"] != 1.0 and rep3["sigma_trans"] != STRANS


# ---- 7. the random walk through the new entries ----
def test_the_random_walk_through_the_new_entries_is_the_old_entries():
    ds, x0, ft = _loop_case("emptied65_gaps")
    rel = fc.rel_motion(65)
    with aar.Problem(ds) as p:
        old = p.track_smooth_fit(x0, SROT, STRANS, frame_time=ft, rel_motion=rel, fit=dict(max_iters=4))
        new = p.track_smooth_fit2(x0, SROT, STRANS, frame_time=ft, rel_motion=rel, fit=dict(max_iters=4))
        t_old, s_old = p.track_smooth_fit_terms(x0, SROT, STRANS, frame_time=ft, rel_motion=rel)
        t_new, s_new = p.track_smooth_fit_terms2(x0, SROT, STRANS, frame_time=ft, rel_motion=rel)
    assert np.array_equal(old[0], new[0]) and np.array_equal(old[2], new[2])
    for k in old[1]:
        assert k == "seconds" or old[1][k] == new[1][k], k
    assert np.array_equal(t_old, t_new) and np.array_equal(s_old, s_new[:4]) and np.all(s_new[4:] == 0.0)


# ---- 8. refusals, 9. NULL arguments, 10. a short report ----
def _raw(p, x0, fit=None, sigma_rot=SROT, cv=CV):
    """both entries through the bare library on pattern-filled outputs: ((rc, message) of the fit, of the terms, everything written nowhere)"""
    L, dp = aar.lib(), aar._dptr
    F = p.ds.num_frames
    x = np.array(p._x(x0), dtype=np.float64)
    keep = np.array(x)
    sp = aar.SmoothParams(sigma_rot, STRANS, None, None, None, **cv)
    fp = aar.smooth_fit_params(**(fit or {}))
    path, terms, sums = np.full(3 * 64, SENT), np.full(4 * max(F, 1), SENT), np.full(6, SENT)
    rep = aar.CSmoothFitReport()
    C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep)
    before = bytes(rep)
    rc = L.aar_track_smooth_fit2(p.handle, dp(x), None, C.byref(sp.c), C.byref(fp), dp(path), C.byref(rep))
    a = (rc, L.aar_last_error().decode())
    rc = L.aar_track_smooth_fit_terms2(p.handle, dp(x), C.byref(sp.c), dp(terms), dp(sums))
    b = (rc, L.aar_last_error().decode())
    untouched = np.array_equal(x, keep) and np.all(path == SENT) and np.all(terms == SENT) and np.all(sums == SENT) and bytes(rep) == before
    return a, b, untouched


def test_refusals_write_nothing():
    ds = aar.synth(2, num_frames=6)
    x0 = sc.track_start(ds)
    with aar.Problem(ds, with_huber=True) as p:
        a, b, untouched = _raw(p, x0)
        for rc, msg in (a, b):
            assert rc == aar.AAR_ERR_UNSUPPORTED and "Huber" in msg and "Gaussian" in msg, msg
        assert untouched
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            a, b, untouched = _raw(p, x0)
            for rc, msg in (a, b):
                assert rc == aar.AAR_ERR_UNSUPPORTED and "single-GPU only" in msg, msg
            assert untouched
    finally:
        comm.close()
        group.close()
    two = aar.synth(2, num_frames=2)
    with aar.Problem(two) as p:
        a, b, untouched = _raw(p, sc.track_start(two))
        for rc, msg in (a, b):
            assert rc == aar.AAR_ERR_INVALID and "num_frames = 2" in msg, msg
        assert untouched
    none = sc.without_frames(ds, range(6))
    assert none.num_obs == 0
    with aar.Problem(none) as p:
        a, b, untouched = _raw(p, x0)
        for rc, msg in (a, b):
            assert rc == aar.AAR_ERR_INVALID and "no detections" in msg, msg
        assert untouched
    with aar.Problem(ds) as p:
        for bad, word in ((dict(estimate_px=0, estimate_rot=0, estimate_trans=0), "estimate"), (dict(rel_tol=-1.0), "rel_tol"),
                          (dict(rel_tol=float("nan")), "rel_tol"), (dict(max_iters=0), "max_iters")):
            a, _, _ = _raw(p, x0, fit=bad)
            assert a[0] == aar.AAR_ERR_INVALID and word in a[1], a
        for kw, word in ((dict(sigma_rot=-1.0), "sigma_rot"), (dict(cv=dict(model=1, sigma_rot0=0.0, sigma_trans0=STRANS0)), "sigma_rot0")):
            a, b, untouched = _raw(p, x0, **kw)
            for rc, msg in (a, b):
                assert rc == aar.AAR_ERR_INVALID and word in msg, msg
            assert untouched
        # ... and the same call goes through once nothing is wrong with it
        a, b, untouched = _raw(p, x0, fit=dict(max_iters=2))
        assert a[0] == 0 and b[0] == 0 and not untouched


def test_null_fit_params_path_and_report_are_accepted():
    ds = aar.synth(2, num_frames=12)
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        x = np.array(p._x(x0), dtype=np.float64)
        sp = aar.SmoothParams(SROT, STRANS, None, None, None, **CV)
        assert aar.lib().aar_track_smooth_fit2(p.handle, aar._dptr(x), None, C.byref(sp.c), None, None, None) == 0
        assert np.array_equal(x, p.track_smooth_fit2(x0, SROT, STRANS, **CV)[0])
        sums = np.zeros(6)
        assert aar.lib().aar_track_smooth_fit_terms2(p.handle, aar._dptr(x), C.byref(sp.c), None, aar._dptr(sums)) == 0
        assert aar.lib().aar_track_smooth_fit_terms2(p.handle, aar._dptr(x), C.byref(sp.c), None, None) == 0
        assert np.array_equal(sums, p.track_smooth_fit_terms2(x, SROT, STRANS, **CV)[1])


def test_a_report_cut_short_by_struct_size():
    ds = aar.synth(2, num_frames=12)
    x0 = sc.track_start(ds)
    cut = aar.CSmoothFitReport.last_rel_change.offset
    with aar.Problem(ds) as p:
        _, full, _ = p.track_smooth_fit2(x0, SROT, STRANS, fit=dict(max_iters=3), **CV)
        x = np.array(p._x(x0), dtype=np.float64)
        sp = aar.SmoothParams(SROT, STRANS, None, None, None, **CV)
        fp = aar.smooth_fit_params(max_iters=3)
        rep = aar.CSmoothFitReport()
        C.memset(C.byref(rep), 0x5A, C.sizeof(rep))
        rep.struct_size = cut
        assert aar.lib().aar_track_smooth_fit2(p.handle, aar._dptr(x), None, C.byref(sp.c), C.byref(fp), None, C.byref(rep)) == 0
    assert rep.struct_size == cut and bytes(rep)[cut:] == b"\x5a" * (C.sizeof(rep) - cut)
    for k in ("iterations", "stop_code", "sigma_px", "sigma_rot", "sigma_trans", "sigma_rot_eff", "sigma_trans_eff"):
        assert getattr(rep, k) == full[k], k


# ---- 11. the fit leaves the model's other entries alone ----
def test_smoothing_and_covariance_bits_are_the_same_before_and_after_a_fit():
    ds, x0, ft = _loop_case("emptied65_gaps")

    def record(p):
        xs, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
        S, R, R2, crep = p.track_smooth_covariance2(xs, SROT, STRANS, frame_time=ft, **CV)
        return [xs, fe, pe, S, R, R2] + [np.array([float(d[k]) for k in sorted(d) if k != "seconds"]) for d in (rep, crep)]

    with aar.Problem(ds) as p:
        before = record(p)
        p.track_smooth_fit2(x0, SROT, STRANS, frame_time=ft, fit=dict(max_iters=3), **CV)
        p.track_smooth_fit_terms2(x0, SROT, STRANS, frame_time=ft, **CV)
        after = record(p)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# ---- 12. the C++ mirror and the driver ----
def _kv(stdout):
    return dict(l.split(" = ") for l in stdout.splitlines() if " = " in l)


def test_mapper_fit_smooth_sigmas_overload(tmp_path):
    exe = str(tmp_path / "smooth_cv_fit_mapper_main")
    cc_ = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_cv_fit_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                          "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS), repr(SROT0), repr(STRANS0)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = _kv(run.stdout)
    ds = aar.synth(2)
    F = ds.num_frames
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, rep, path = p.track_smooth_fit2(xt, SROT, STRANS, frame_time=np.asarray(ds.frame_ids, dtype=np.float64), **CV)
    assert int(kv["iterations"]) == rep["iterations"] and int(kv["stop_code"]) == rep["stop_code"] and int(kv["rows"]) == rep["iterations"] + 1
    # (the mapper carries its poses as 4x4 matrices between its calls: a few ulps of the start, 1e-8 in the poses; the sigmas follow the track)
    for k in ("sigma_px", "sigma_rot", "sigma_trans", "sigma_rot_eff", "sigma_trans_eff"):
        np.testing.assert_allclose(float(kv[k]), rep[k], rtol=1e-6, err_msg=k)
    np.testing.assert_allclose(np.array([float(v) for v in kv["path"].split()]).reshape(-1, 3), path, rtol=1e-6)
    z = np.array([float(v) for v in kv["z"].split()]).reshape(F, 6)
    zs = _frames(ds, xs)
    assert np.abs(z[:, 3:] - zs[:, 3:]).max() < 1e-6 and np.abs(tr.rodrigues(z[:, :3]) - tr.rodrigues(zs[:, :3])).max() < 1e-6


def _cli_folder(root):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = os.path.join(root, "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # the first 90 frames, as tests/test_gpu_smooth_fit.py cuts the recording: the later ones turn through pi, where the solution file's
    # vec -> matrix -> vec round trip lands on another rotation vector
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    return exe, folder, [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]


def test_find_solution_cv_fit_sigmas_switch(tmp_path):
    exe, folder, base = _cli_folder(str(tmp_path))
    env = dict(os.environ, AAR_DETERMINISTIC="1")
    run = subprocess.run(base, capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "smooth-cv-fit: " not in run.stdout, run.stdout + run.stderr
    solved = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    run = subprocess.run(base + ["-smooth", repr(SROT), repr(STRANS), "-cv", repr(SROT0), repr(STRANS0), "-cv-fit-sigmas"], capture_output=True,
                         text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("smooth-cv-fit: ")]
    assert len(line) == 1 and "smooth: constant velocity" in run.stdout and "smooth-fit: " not in run.stdout, run.stdout
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    ft = np.asarray(solved.frame_ids, dtype=np.float64)
    n0 = sc.ns(solved)
    with aar.Problem(solved) as p:
        xt, _, _ = p.track(solved.x_full, aar.lm_default_params())
        xf, rep, _ = p.track_smooth_fit2(xt, SROT, STRANS, frame_time=ft, **CV)
        xs, _, _, _ = p.track_smooth(xf, rep["sigma_rot_eff"], rep["sigma_trans_eff"], frame_time=ft, model=1,
                                     sigma_rot0=SROT0 / rep["sigma_px"], sigma_trans0=STRANS0 / rep["sigma_px"])
    words = line[0].split()
    for k in ("sigma_px", "sigma_rot", "sigma_trans", "sigma_rot_eff", "sigma_trans_eff"):
        np.testing.assert_allclose(float(words[words.index(k) + 1]), rep[k], rtol=1e-6, err_msg=k)
    np.testing.assert_allclose(float(words[words.index("sigma_rot0_eff") + 1]), SROT0 / rep["sigma_px"], rtol=1e-6)
    assert int(words[words.index("after") + 1]) == rep["iterations"]
    assert np.abs(got.x_full - xs).max() < 1e-6
    assert np.abs(got.x_full[n0:] - solved.x_full[n0:]).max() > 1e-6


def test_find_solution_refuses_cv_fit_sigmas_without_its_switches(tmp_path):
    exe, folder, base = _cli_folder(str(tmp_path))
    sm, cv = ["-smooth", "0.05", "0.02"], ["-cv", "1", "1"]
    # without -cv, without -smooth, with -live; and -cv ... -fit-sigmas stays refused
    for bad in (base + sm + ["-cv-fit-sigmas"], base + cv + ["-cv-fit-sigmas"], base + ["-cv-fit-sigmas"],
                base + ["-live", "0"] + cv + ["-cv-fit-sigmas"], base + ["-live", "2", "0.05", "0.02"] + cv + ["-cv-fit-sigmas"],
                base + sm + cv + ["-fit-sigmas"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-cv-fit-sigmas" in run.stdout and "smooth-cv-fit: " not in run.stdout and "smooth: " not in run.stdout, run.stdout
