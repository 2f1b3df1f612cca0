"""Smoothed tracking under the constant-velocity prior (aar_track_smooth with AAR_SMOOTH_MODEL_CONSTANT_VELOCITY, DESIGN.md section 31: a
second-difference prior, block-pentadiagonal H, every try a cyclic reduction on pairs of frames) against the float64 restatement
tests/smooth_cv_restated.py.  Needs a real MI355X.

Bars: blocks and right-hand side 1e-12 of the largest entry (section 16's); the damped step max(10 eps cond_2(H + mu I), 1e-13) relative in the
infinity norm against the banded solve (section 28's convention, the floor for the two solves' own rounding); the reduction by residual
1e-10 |b|_inf at every shape; LM runs: equal iteration and rejected-try counts on cases whose every decision the restated run decides (margin
above 1e-9), poses 1e-9.
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_cv_restated as cv
import smooth_restated as sr
import track_restated as tr
from conftest import PKG, ROOT, load_golden

pytestmark = pytest.mark.gpu

SROT, STRANS = cc.SROT, cc.STRANS
CV = dict(model="cv", sigma_rot0=cc.SROT0, sigma_trans0=cc.STRANS0)
T = 16                       # SMOOTH_CV_T of csrc/kernels.h: a level with more eliminating supernodes than this is a launch of its own
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _problem(ds, delta=None, **kw):
    p = aar.Problem(ds, with_huber=delta is not None, **kw)
    if delta is not None:
        p.set_huber_delta(delta)
    return p


def _restated(td, delta=None, frame_time=None):
    return cv.SmoothCvProblem(td, SROT, STRANS, cc.SROT0, cc.STRANS0, delta=delta, frame_time=frame_time)


# ---- 1. the system of one try ----
@pytest.mark.parametrize("variant", ["plain", "uneven_emptied"])
@pytest.mark.parametrize("start", [0, 1, 2])
def test_system_of_one_try(start, variant):
    F = 12
    ds = aar.synth(2, num_frames=F)
    x0 = sc.track_start(ds)
    if start:                                        # the data set's perturbed start, and two more on top of it
        rng = np.random.default_rng(100 + start)
        x0[sc.ns(ds):] += (rng.normal(size=(F, 6)) * [0.03, 0.03, 0.03, 0.01, 0.01, 0.01]).reshape(-1)
    ft = None
    if variant == "uneven_emptied":
        ds = sc.without_frames(ds, [0, 5, 6, F - 1])
        ft = cc.gaps(F)
    td = tr.TrackData(ds, x0)
    sp = _restated(td, frame_time=ft)
    diag, off, off2, rhs = sp.system(td.z0)
    Ef, Pe = sp.costs(td.z0)
    H = cv.dense(diag, off, off2)
    mu0 = float(np.max(np.einsum("fii->fi", diag)))
    with aar.Problem(ds) as p:
        for mu in (mu0, 1e-3 * mu0):
            d_ref = cv.solve(diag, off, off2, rhs, mu)
            gd, go, go2, gr, gdel, cost = p.track_smooth_system2(x0, SROT, STRANS, mu, frame_time=ft, **CV)
            big = max(np.abs(diag).max(), np.abs(off).max(), np.abs(off2).max())
            e_blk = max(np.abs(gd - diag).max(), np.abs(go - off).max(), np.abs(go2 - off2).max()) / big
            e_rhs = np.abs(gr - rhs).max() / np.abs(rhs).max()
            e_del = np.abs(gdel - d_ref).max() / np.abs(d_ref).max()
            bar = max(10 * EPS * np.linalg.cond(H + mu * np.eye(len(rhs))), 1e-13)
            print("start %d %s mu %.3g: blocks %.2e rhs %.2e delta %.2e (bar %.2e)" % (start, variant, mu, e_blk, e_rhs, e_del, bar))
            assert e_blk <= 1e-12 and e_rhs <= 1e-12, (e_blk, e_rhs)
            assert e_del <= bar, (e_del, bar)
            np.testing.assert_allclose(cost, [Ef.sum(), Pe.sum()], rtol=1e-11)
    assert np.abs(off2).max() > 0


# ---- 2. shapes of the reduction ----
def _shape_dataset(F):
    cfg = 2 if F <= 65 else 3 if F <= 131 else 4 if F <= 2000 else 5
    ds = aar.synth(cfg, num_frames=F)
    return sc.without_frames(ds, sc.emptied(F))


def _launches(F):
    """one launch while every level fits the finishing workgroup, else damping + tail + a level and a back-substitution per own level"""
    K, n, s = (F + 1) // 2, 0, 1
    while s < K and -(-K // (2 * s)) > T:
        n, s = n + 1, 2 * s
    return 2 * n + 2 if n else 1


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 6, 7, 8, 9, 4 * T - 1, 4 * T, 4 * T + 1, 4 * T + 2, 8 * T + 3, 2000, 5000])
def test_shapes_of_the_reduction(F):
    ds = _shape_dataset(F)
    assert ds.num_frames == F
    x0 = sc.track_start(ds)
    ft = cc.gaps(F) if F > 1 else None
    with aar.Problem(ds) as p:
        gd, go, go2, gr, _, _ = p.track_smooth_system2(x0, SROT, STRANS, 1.0, frame_time=ft, **CV)
        mu0 = float(np.max(np.einsum("fii->fi", gd)))
        for mu in (mu0, 1e-3 * mu0):
            d = p.track_smooth_system2(x0, SROT, STRANS, mu, frame_time=ft, **CV)[4]
            assert np.all(np.isfinite(d))           # (a NaN in the padded supernode of an odd F would reach its neighbours' entries)
            res = np.abs(cv.matvec(gd, go, go2, d, mu) - gr).max() / np.abs(gr).max()
            print("F %d mu %.3g: residual %.2e" % (F, mu, res))
            assert res <= 1e-10, res
    assert aar.smooth_solve_launches(F, "cv") == _launches(F)
    assert [_launches(n) for n in (4 * T, 4 * T + 1, 8 * T, 8 * T + 1, 8 * T + 3)] == [1, 4, 4, 6, 6]


# ---- 3. LM runs against the restated LM ----
def _lm_case(name):
    kw, lm, delta = {}, {}, None
    ds = aar.synth(2, num_frames=40, **(dict(init_scale=25.0) if name == "far" else {}))
    x0 = sc.track_start(ds)
    if name == "far":
        lm = dict(tau=1e-6)
    if name == "gap":
        ds = sc.without_frames(ds, sc.emptied(40))
    if name == "huber":
        delta = 0.5
    if name == "uneven":
        kw = dict(frame_time=cc.gaps(40))
    return ds, x0, delta, kw, lm


@pytest.mark.parametrize("name", ["plain", "gap", "far", "huber", "uneven"])
def test_lm_against_the_restated_lm(name):
    ds, x0, delta, kw, lm = _lm_case(name)
    td = tr.TrackData(ds, x0)
    sp = _restated(td, delta=delta, **kw)
    r = cv.smooth_lm(sp, td.z0, **lm)
    print(name, {k: v for k, v in r.items() if k != "z"})
    assert r["margin"] > 1e-9                      # the case itself must be decided
    if name == "far":
        assert r["rejected"] > 0
    if name == "huber":
        assert sum(tr.weighted(sp.fd[f], r["z"][f], delta)[1].sum() for f in range(sp.F)) > 0
    with _problem(ds, delta) as p:
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, params=aar.lm_default_params(**lm), **kw, **CV)
    n0 = sc.ns(ds)
    assert np.array_equal(x[:n0], x0[:n0])          # cameras and markers bit-unchanged
    assert rep["iterations"] == r["iterations"] and rep["rejected_tries"] == r["rejected"] and rep["stop_code"] == r["exit"]
    np.testing.assert_allclose(rep["final_cost"], r["err"], rtol=1e-10)
    dz = np.abs(x[n0:].reshape(-1, 6) - r["z"]).max()
    print(name, "pose difference %.2e" % dz)
    assert dz < 1e-9, dz
    Ef, Pe = sp.costs(r["z"])
    np.testing.assert_allclose(fe, Ef, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(pe, Pe, rtol=1e-7, atol=1e-12)      # entry 0 is pair 0, entry f term f
    np.testing.assert_allclose(fe.sum() + pe.sum(), rep["final_cost"], rtol=1e-12)


# ---- 4. the claim on the device ----
def test_claim_case_ends_at_the_restated_poses():
    ds, x0, empty = cc.claim_case()
    td = tr.TrackData(ds, x0)
    r = cv.smooth_lm(_restated(td), td.z0, **cc.TIGHT)
    assert r["margin"] > 1e-9
    prm = aar.lm_default_params(min_average_step_error_diff=cc.TIGHT["min_avg"], max_iters=cc.TIGHT["max_iters"])
    with aar.Problem(ds) as p:
        x, rep, _, _ = p.track_smooth(x0, SROT, STRANS, params=prm, **CV)
        xr, _, _, _ = p.track_smooth(x0, SROT, STRANS, params=prm)
    z = x[sc.ns(ds):].reshape(-1, 6)
    dz = np.abs(z - r["z"]).max()
    e_cv, e_rw = cc.end_errors(z, ds), cc.end_errors(xr[sc.ns(ds):], ds)
    print("claim case: pose difference %.2e, %d iterations; end frames cv %.3e %.3e, rw %.3e %.3e" % ((dz, rep["iterations"]) + e_cv + e_rw))
    assert rep["iterations"] == r["iterations"] and dz < 1e-9, dz
    assert e_cv[0] <= 0.5 * e_rw[0] and e_cv[1] <= 0.5 * e_rw[1]      # (tests/test_smooth_cv_host.py on the restatement, carried over)


# ---- 5. model switch and reproducibility ----
REPORT_KEYS = ("iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost", "final_prior_cost", "final_mu")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and all(a[1][k] == b[1][k] for k in REPORT_KEYS)


def test_model_switch_and_reproducibility():
    ds, g = load_golden("g_track_cfg2_huber")
    x0 = np.array(g["track_x0"])
    ft = cc.gaps(ds.num_frames)
    with _problem(ds, 10.0) as p:
        t0 = p.track(x0, aar.lm_default_params())
        short = p.track_smooth(x0, SROT, STRANS, frame_time=ft)                              # the 40-byte struct
        long0 = p.track_smooth(x0, SROT, STRANS, frame_time=ft, model="rw", sigma_rot0=-1.0)   # the long one, model = 0
        a = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
        b = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
        s_short = p.track_smooth_system(x0, SROT, STRANS, 1.0, frame_time=ft)
        s_long = p.track_smooth_system2(x0, SROT, STRANS, 1.0, frame_time=ft, model="rw")
        t1 = p.track(x0, aar.lm_default_params())
    assert _same(short, long0)                       # the random walk has not moved, bit for bit
    assert _same(a, b) and a[1]["iterations"] > 1    # two constant-velocity calls give the same bits
    assert not np.array_equal(a[0], short[0])
    for u, v in zip(s_short[:2] + s_short[2:4], s_long[:2] + s_long[3:5]):
        assert np.array_equal(u, v)
    assert s_long[2].shape == (ds.num_frames - 2, 6, 6) and not s_long[2].any()   # off2 is zero under the random walk
    for u, v in zip(t0, t1):                         # aar_track is unaffected
        assert np.array_equal(u, v)


# ---- 6. refusals ----
def _sentinel(n):
    return np.full(max(n, 1), -7.25)


def _refused(call, bufs, word):
    rc = call()
    msg = aar.lib().aar_last_error().decode()
    assert rc == aar.AAR_ERR_UNSUPPORTED, (rc, msg)
    assert word in msg, msg
    for b in bufs:
        assert np.all(b == -7.25)                    # nothing written


def test_other_entries_refuse_constant_velocity():
    ds, g = load_golden("g_track_cfg2")
    x0 = np.array(g["track_x0"])
    F = ds.num_frames
    L = aar.lib()
    dp = aar._dptr
    with aar.Problem(ds) as p:
        x = np.array(p._x(x0), dtype=np.float64)
        sp = aar.SmoothParams(SROT, STRANS, None, None, None, **CV)
        ref = C.byref(sp.c)
        word = "AAR_SMOOTH_MODEL_CONSTANT_VELOCITY"
        b = [_sentinel(36 * F), _sentinel(36 * F), _sentinel(6 * F), _sentinel(6 * F), _sentinel(2)]
        _refused(lambda: L.aar_track_smooth_system(p.handle, dp(x), ref, 1.0, dp(b[0]), dp(b[1]), dp(b[2]), dp(b[3]), dp(b[4])), b, "aar_track_smooth_system2")
        b = [_sentinel(36 * F), _sentinel(36 * F)]
        rep = aar.CSmoothCovarianceReport()
        rep.struct_size = C.sizeof(rep)
        _refused(lambda: L.aar_track_smooth_covariance(p.handle, dp(x), ref, dp(b[0]), dp(b[1]), C.byref(rep)), b, word)
        assert rep.num_vars == 0 and rep.launches == 0
        b = [_sentinel(4 * F), _sentinel(4)]
        _refused(lambda: L.aar_track_smooth_fit_terms(p.handle, dp(x), ref, dp(b[0]), dp(b[1])), b, word)
        xs, path = np.array(x), _sentinel(3 * 64)
        frep = aar.CSmoothFitReport()
        frep.struct_size = C.sizeof(frep)
        _refused(lambda: L.aar_track_smooth_fit(p.handle, dp(xs), None, ref, None, dp(path), C.byref(frep)), [path], word)
        assert np.array_equal(xs, x) and frep.iterations == 0
        qt = np.array([0.5, 1.5])
        b = [_sentinel(12), _sentinel(72)]
        seg = np.full(2, -9, dtype=np.int32)
        _refused(lambda: L.aar_track_smooth_query(p.handle, dp(x), ref, 2, dp(qt), dp(b[0]), dp(b[1]), seg.ctypes.data_as(C.POINTER(C.c_int32)), None), b, word)
        assert np.all(seg == -9)
        # rel_motion under constant velocity is refused by the entry points as the validator refuses it
        with pytest.raises(aar.AarError) as e:
            p.track_smooth(x0, SROT, STRANS, rel_motion=np.zeros((F - 1, 6)), **CV)
        assert e.value.code == aar.AAR_ERR_INVALID and "rel_motion" in str(e.value)


def test_unsupported_behind_a_communicator():
    ds, g = load_golden("g_track_cfg2")
    x0 = np.array(g["track_x0"])
    world = 2
    group = aar.LocalGroup(world)
    out = [None] * world

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with aar.Problem(ds, comm=comm) as p:
                codes = []
                for call in (lambda: p.track_smooth(x0, SROT, STRANS, **CV), lambda: p.track_smooth_system2(x0, SROT, STRANS, 1.0, **CV)):
                    try:
                        call()
                        codes.append(0)
                    except aar.AarError as e:
                        codes.append(e.code)
                out[r] = codes
        except Exception as e:   # noqa: BLE001
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
    assert out == [[aar.AAR_ERR_UNSUPPORTED] * 2] * world, out


def test_degenerate_sizes_return_cleanly():
    ds = aar.synth(2, num_frames=6)
    none = sc.without_frames(ds, range(6))            # no detection anywhere: the prior alone
    assert none.num_obs == 0
    with aar.Problem(none) as p:
        x, rep, fe, pe = p.track_smooth(sc.track_start(none), SROT, STRANS, **CV)
    assert np.all(np.isfinite(x)) and np.all(fe == 0.0) and rep["final_data_cost"] == 0.0 and rep["final_cost"] <= rep["initial_cost"]
    one = aar.synth(2, num_frames=1)                  # no pair: one frame of the joint LM, what the random walk gives
    x0 = sc.track_start(one)
    with aar.Problem(one) as p:
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, **CV)
        xr, repr_, _, _ = p.track_smooth(x0, SROT, STRANS)
        assert p.track_smooth_system2(x0, SROT, STRANS, 1.0, **CV)[2].shape == (0, 6, 6)
    assert len(pe) == 0 and rep["final_prior_cost"] == 0.0 and rep["iterations"] == repr_["iterations"]
    assert np.abs(x - xr).max() < 1e-9
    two = aar.synth(2, num_frames=2)                  # pair 0 alone: the random walk with pair 0's sigmas
    x0 = sc.track_start(two)
    with aar.Problem(two) as p:
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, **CV)
        xr, repr_, _, per = p.track_smooth(x0, cc.SROT0, cc.STRANS0)
    assert len(pe) == 1 and rep["iterations"] == repr_["iterations"]
    assert np.abs(x - xr).max() < 1e-9
    np.testing.assert_allclose(pe, per, rtol=1e-6, atol=1e-15)
    single_empty = sc.without_frames(one, [0])        # F = 1 and nothing seen: rows = 0, nothing to do
    x0 = sc.track_start(one)
    with aar.Problem(single_empty) as p:
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, **CV)
    assert np.array_equal(x, x0) and rep["iterations"] == 0


def test_no_frames_at_all():
    ds = aar.synth(2, num_frames=2)
    n0 = sc.ns(ds)
    z = np.zeros(0, dtype=np.int32)
    empty = sc.copy_of(ds, num_frames=0, frame_ids=z, obs_frame=z, obs_cam=z, obs_marker=z, obs_uv=np.zeros((0, 8), dtype=np.float32),
                       x_full=np.array(ds.x_truth[:n0]), x_truth=np.array(ds.x_truth[:n0]))
    with aar.Problem(empty) as p:
        x, rep, fe, pe = p.track_smooth(empty.x_full, SROT, STRANS, **CV)
        blocks = p.track_smooth_system2(empty.x_full, SROT, STRANS, 1.0, **CV)
    assert np.array_equal(x, empty.x_full) and rep["iterations"] == 0 and len(fe) == 0 and len(pe) == 0
    assert all(len(b) == 0 for b in blocks[:5]) and blocks[5] == (0.0, 0.0)


# ---- 7. callers ----
def test_mapper_track_smooth_overload(tmp_path):
    exe = str(tmp_path / "smooth_cv_mapper_main")
    cc_ = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_cv_mapper_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                          "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS), repr(cc.SROT0), repr(cc.STRANS0)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = dict(l.split(" = ") for l in run.stdout.splitlines() if " = " in l)
    ds = aar.synth(2)
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        xt, _, et = p.track(x0, aar.lm_default_params())
        xs, rep, fe, pe = p.track_smooth(xt, SROT, STRANS, frame_time=np.asarray(ds.frame_ids, dtype=np.float64), **CV)
        xr, _, _, _ = p.track_smooth(xt, SROT, STRANS, frame_time=np.asarray(ds.frame_ids, dtype=np.float64))
    assert int(kv["frames"]) == ds.num_frames and int(kv["pairs"]) == ds.num_frames - 1
    assert int(kv["iterations"]) == rep["iterations"] and int(kv["stop_code"]) == rep["stop_code"]
    np.testing.assert_allclose(float(kv["final_cost"]), rep["final_cost"], rtol=1e-9)
    np.testing.assert_allclose([float(kv["sum_frame_err"]), float(kv["sum_pair_err"])], [fe.sum(), pe.sum()], rtol=1e-8)
    z = np.array([[float(v) for v in kv["z%d" % f].split()] for f in range(ds.num_frames)])
    # (the mapper carries its poses as 4x4 matrices between the two calls: the round trip costs a few ulps of the start)
    assert np.abs(z - xs[sc.ns(ds):].reshape(-1, 6)).max() < 1e-8
    assert np.abs(z - xr[sc.ns(ds):].reshape(-1, 6)).max() > 1e-6       # and not the random walk's


def test_find_solution_cv_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    os.replace(os.path.join(folder, "initial.solution"), os.path.join(folder, "initial_tracking_only.solution"))
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only", "-smooth", "0.05", "0.02"]
    got = {}
    for flag in ([], ["-cv", "1", "1"]):
        run = subprocess.run(base + flag, capture_output=True, text=True, timeout=300, env=dict(os.environ, AAR_DETERMINISTIC="1"))
        assert run.returncode == 0, run.stdout + run.stderr
        assert "smooth: " in run.stdout and ("smooth: constant velocity" in run.stdout) == bool(flag)
        got[bool(flag)] = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    n0 = sc.ns(got[True])
    assert np.abs(got[True].x_full[:n0] - got[False].x_full[:n0]).max() < 1e-12      # cameras and markers are the solve's
    assert np.abs(got[True].x_full[n0:] - got[False].x_full[n0:]).max() > 1e-6       # the frames differ between the models
    # refused with the usage message: without -smooth, with one sigma, with a non-positive one, with the entries that need the selected inverse
    no_smooth = [exe, folder, "0.05", "x", "-from-initial", "-tracking-only", "-cv", "1", "1"]
    for bad in (no_smooth, base + ["-cv", "1"], base + ["-cv", "1", "-1"], base + ["-cv", "1", "1", "-smooth-covariance"],
                base + ["-cv", "1", "1", "-fit-sigmas"], base + ["-cv", "1", "1", "-resample", "4"], base + ["-resample", "4", "-cv", "1", "1"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "smooth: " not in run.stdout, run.stdout
