"""Smoothed tracking (aar_track_smooth: track()'s data terms tied by a motion prior between consecutive frames, one joint LM on the device,
every try a block cyclic reduction) against the float64 restatement tests/smooth_restated.py.  Needs a real MI355X.

Bars: blocks and right-hand side 1e-12 of the largest entry (the project's J^T J bar); the damped step 1e-8 relative in the infinity norm
against the banded solve (the project's bar for direct solves), by residual 1e-10 |b|_inf above 500 frames; LM runs as tests/test_gpu_track.py
holds track(): equal iteration and rejected-try counts, final cost rtol 1e-10, poses 1e-9 + 2 slack.
"""
import os
import subprocess
import threading

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_restated as sr
import track_restated as tr
from conftest import PKG, ROOT, load_golden

pytestmark = pytest.mark.gpu

SROT, STRANS = 0.05, 0.02      # rad, metre per sqrt(frame): a prior of the data's own weight at configs 2-4 (prior cost ~ 1/3 of the data cost)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _golden_track(name):
    ds, g = load_golden(name)
    ds.x_full = np.array(g["track_x0"])
    return ds, g


def _gaps(F):
    """frame times with a hole of five every seventh frame"""
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(F - 1) % 7 == 3) * 4.0])


def _truth_rel(ds):
    """the truth's own relative motions: what odometry would feed"""
    z = ds.x_truth[sc.ns(ds): sc.ns(ds) + 6 * ds.num_frames].reshape(-1, 6)
    return np.stack([np.r_[sr.so3_log(tr.rodrigues(z[f, :3]).T @ tr.rodrigues(z[f + 1, :3])), z[f + 1, 3:] - z[f, 3:]]
                     for f in range(ds.num_frames - 1)])


def _problem(ds, delta=None, **kw):
    p = aar.Problem(ds, with_huber=delta is not None, **kw)
    if delta is not None:
        p.set_huber_delta(delta)
    return p


# ---- 1. the system of one try ----
def _system_inputs():
    out = []
    ds, _ = load_golden("g2_small")
    out.append(("g2_small", ds, np.array(ds.x_full), None))
    ds, _ = _golden_track("g_track_cfg2")
    out.append(("g_track_cfg2", ds, np.array(ds.x_full), None))
    ds, _ = _golden_track("g_track_cfg2_huber")
    out.append(("g_track_cfg2_huber", ds, np.array(ds.x_full), 10.0))
    return out


@pytest.mark.parametrize("variant", ["plain", "gaps", "rel", "gaps_rel"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_system_of_one_try(which, variant):
    name, ds, x0, delta = _system_inputs()[which]
    F = ds.num_frames
    ft = _gaps(F) if "gaps" in variant else None
    rng = np.random.default_rng(3)
    rel = rng.normal(size=(F - 1, 6)) * [0.05, 0.05, 0.05, 0.02, 0.02, 0.02] if "rel" in variant else None
    td = tr.TrackData(ds, x0)
    sp = sr.SmoothProblem(td, SROT, STRANS, delta=delta, frame_time=ft, rel_motion=rel)
    diag, off, rhs = sp.system(td.z0)
    Ef, Pe = sp.costs(td.z0)
    mu0 = float(np.max(np.einsum("fii->fi", diag)))
    with _problem(ds, delta) as p:
        for mu in (mu0, 1e-3 * mu0):
            d_ref = sr.solve(diag, off, rhs, mu)
            # the restatement's own solve against long double refinement: an input it cannot solve to 1e-9 is no yardstick for 1e-8
            A = (sr.dense(diag, off) + mu * np.eye(len(rhs)))
            x = d_ref.astype(np.longdouble)
            for _ in range(4):
                x = x + np.linalg.solve(A, (rhs.astype(np.longdouble) - A.astype(np.longdouble) @ x).astype(np.float64))
            assert float(np.abs(d_ref - x).max() / np.abs(x).max()) < 1e-9
            gd, go, gr, gdel, cost = p.track_smooth_system(x0, SROT, STRANS, mu, frame_time=ft, rel_motion=rel)
            big = max(np.abs(diag).max(), np.abs(off).max())
            e_blk = max(np.abs(gd - diag).max(), np.abs(go - off).max()) / big
            e_rhs = np.abs(gr - rhs).max() / np.abs(rhs).max()
            e_del = np.abs(gdel - d_ref).max() / np.abs(d_ref).max()
            print("%s %s mu %.3g: blocks %.2e rhs %.2e delta %.2e" % (name, variant, mu, e_blk, e_rhs, e_del))
            assert e_blk < 1e-12 and e_rhs < 1e-12, (e_blk, e_rhs)
            assert e_del < 1e-8, e_del
            np.testing.assert_allclose(cost, [Ef.sum(), Pe.sum()], rtol=1e-11)
            assert np.array_equal(gd, np.swapaxes(gd, 1, 2))           # the diagonal blocks are stored symmetric


# ---- 2. shapes of the reduction ----
def _shape_dataset(F):
    cfg = 2 if F <= 65 else 3 if F <= 127 else 4 if F <= 2000 else 5
    ds = aar.synth(cfg, num_frames=F)
    return sc.without_frames(ds, sc.emptied(F))


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 63, 64, 65, 127, 500, 2000, 5000])
def test_shapes_of_the_reduction(F):
    ds = _shape_dataset(F)
    assert ds.num_frames == F
    x0 = sc.track_start(ds)
    ft = _gaps(F) if F > 1 else None
    with aar.Problem(ds) as p:
        gd, go, gr, _, _ = p.track_smooth_system(x0, SROT, STRANS, 1.0, frame_time=ft)
        mu0 = float(np.max(np.einsum("fii->fi", gd)))
        for mu in (mu0, 1e-3 * mu0):
            d = p.track_smooth_system(x0, SROT, STRANS, mu, frame_time=ft)[3]
            res = np.abs(sr.matvec(gd, go, d, mu) - gr).max() / np.abs(gr).max()
            if F <= 500:
                d_ref = sr.solve(gd, go, gr, mu)
                err = np.abs(d - d_ref).max() / np.abs(d_ref).max()
                print("F %d mu %.3g: delta %.2e residual %.2e" % (F, mu, err, res))
                assert err < 1e-8, err
            else:
                print("F %d mu %.3g: residual %.2e" % (F, mu, res))
            assert res <= 1e-10, res
    empty = sc.emptied(F)
    if empty:
        cnt = np.bincount(ds.obs_frame, minlength=F)
        assert np.all(cnt[empty] == 0) and (F < 30 or len(empty) == 12)


def test_degenerate_sizes_return_cleanly():
    ds = aar.synth(2, num_frames=6)
    none = sc.without_frames(ds, range(6))            # no detection anywhere: the prior alone
    assert none.num_obs == 0
    with aar.Problem(none) as p:
        x, rep, fe, pe = p.track_smooth(sc.track_start(none), SROT, STRANS)
    assert np.all(np.isfinite(x)) and np.all(fe == 0.0) and rep["final_data_cost"] == 0.0 and rep["final_cost"] <= rep["initial_cost"]
    one = aar.synth(2, num_frames=1)                  # no pair: one frame of the joint LM
    x0 = sc.track_start(one)
    td = tr.TrackData(one, x0)
    r = sr.smooth_lm(sr.SmoothProblem(td, SROT, STRANS), td.z0)
    with aar.Problem(one) as p:
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS)
    assert len(pe) == 0 and rep["iterations"] == r["iterations"] and rep["final_prior_cost"] == 0.0
    np.testing.assert_allclose(rep["final_cost"], r["err"], rtol=1e-10)
    assert np.abs(x[sc.ns(one):] - r["z"].reshape(-1)).max() < 1e-9 + 2 * r["slack"]
    single_empty = sc.without_frames(one, [0])        # F = 1 and nothing seen: rows = 0, nothing to do
    with aar.Problem(single_empty) as p:
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS)
    assert np.array_equal(x, x0) and rep["iterations"] == 0


# ---- 3. LM runs against the restated LM ----
# margins of the restated runs, measured on the CPU while writing this test (all far above MARGIN = 1e-9):
#   plain 3.9e-4, gap (with emptied frames) 8.1e-4, far x20 1.2e-3, far x20 tau 1e-6 (8 rejected tries) 1.2e-3, huber 0.5 px 6.1e-4, rel 1.5e-3
def _lm_case(name):
    kw, lm, delta = {}, {}, None
    if name in ("far", "far_tau"):
        ds = aar.synth(2, num_frames=40, init_scale=20.0)
        if name == "far_tau":
            lm = dict(tau=1e-6)
    else:
        ds = aar.synth(2, num_frames=40)
    x0 = sc.track_start(ds)
    srot, strans = SROT, STRANS
    if name == "gap":
        ds = sc.without_frames(ds, sc.emptied(40))
        kw = dict(frame_time=_gaps(40))
    if name == "huber":
        delta = 0.5
    if name == "rel":
        kw = dict(rel_motion=_truth_rel(ds))
        srot, strans = 0.01, 0.005
    return ds, x0, srot, strans, delta, kw, lm


@pytest.mark.parametrize("name", ["plain", "gap", "far", "far_tau", "huber", "rel"])
def test_lm_against_the_restated_lm(name):
    ds, x0, srot, strans, delta, kw, lm = _lm_case(name)
    td = tr.TrackData(ds, x0)
    sp = sr.SmoothProblem(td, srot, strans, delta=delta, **kw)
    r = sr.smooth_lm(sp, td.z0, **lm)
    print(name, {k: v for k, v in r.items() if k != "z"})
    assert r["margin"] > 1e-9                      # nothing may be excluded from a joint run: the case itself must be decided
    if name == "far_tau":
        assert r["rejected"] > 0
    if name == "huber":
        assert sum(tr.weighted(sp.fd[f], r["z"][f], delta)[1].sum() for f in range(sp.F)) > 0
    with _problem(ds, delta) as p:
        x, rep, fe, pe = p.track_smooth(x0, srot, strans, params=aar.lm_default_params(**lm), **kw)
    n0 = sc.ns(ds)
    assert np.array_equal(x[:n0], x0[:n0])          # cameras and markers bit-unchanged
    assert rep["iterations"] == r["iterations"] and rep["rejected_tries"] == r["rejected"] and rep["stop_code"] == r["exit"]
    np.testing.assert_allclose(rep["final_cost"], r["err"], rtol=1e-10)
    np.testing.assert_allclose([rep["final_data_cost"], rep["final_prior_cost"]], [r["data"], r["prior"]], rtol=1e-9)
    dz = np.abs(x[n0:].reshape(-1, 6) - r["z"]).max()
    print(name, "pose difference %.2e" % dz)
    assert dz < 1e-9 + 2 * r["slack"], dz
    Ef, Pe = sp.costs(r["z"])
    np.testing.assert_allclose(fe, Ef, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(pe, Pe, rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(fe.sum() + pe.sum(), rep["final_cost"], rtol=1e-12)


# ---- 4. bridging ----
def test_emptied_frames_are_bridged():
    ds0 = aar.synth(2, num_frames=40)
    hole = list(range(14, 19))
    ds = sc.without_frames(ds0, hole)
    x0 = sc.track_start(ds)
    n0 = sc.ns(ds)
    tight = dict(min_average_step_error_diff=0.0, max_iters=60)
    with aar.Problem(ds) as p:
        xt, it, _ = p.track(x0, aar.lm_default_params())
        xs, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, params=aar.lm_default_params(**tight))
    for f in hole:                                   # the contrast: track() leaves them bit-unchanged
        assert it[f] == 0 and np.array_equal(xt[n0 + 6 * f: n0 + 6 * f + 6], x0[n0 + 6 * f: n0 + 6 * f + 6])
    td = tr.TrackData(ds, x0)
    r = sr.smooth_lm(sr.SmoothProblem(td, SROT, STRANS), td.z0, min_avg=0.0, max_iters=60)
    zs = xs[n0:].reshape(-1, 6)
    # two runs to the same minimiser with the average-step stop off: the bar of the LM runs (the last, rounding-level steps of either run
    # may or may not be taken: measured slack 6e-6 on the CPU)
    assert np.abs(zs - r["z"]).max() < 1e-9 + 2 * r["slack"], (np.abs(zs - r["z"]).max(), r["slack"])
    # a random walk with equal gaps, the neighbours held: the emptied frames lie on the geodesic between frames 13 and 19
    for f in hole:
        g = sr.geodesic(zs[13], zs[19], (f - 13) / 6.0)
        assert np.abs(zs[f] - g).max() < 1e-6, (f, np.abs(zs[f] - g).max())
        assert np.abs(zs[f] - x0[n0 + 6 * f: n0 + 6 * f + 6]).max() > 1e-4 and fe[f] == 0.0


# ---- 5. minimiser property ----
def test_result_is_a_minimiser():
    ds = aar.synth(3, num_frames=127)
    x0 = sc.track_start(ds)
    tight = aar.lm_default_params(min_average_step_error_diff=0.0, max_iters=100)
    with aar.Problem(ds) as p:
        xt, _, et = p.track(x0, tight)
        b0 = p.track_smooth_system(x0, SROT, STRANS, 1.0)[2]
        xs, rep, fe, pe = p.track_smooth(x0, SROT, STRANS, params=tight)
        b1 = p.track_smooth_system(xs, SROT, STRANS, 1.0)[2]
        cost_t = p.track_smooth_system(xt, SROT, STRANS, 1.0)[4]
    print("E(smooth) %.6f, E(track) %.6f, gradient %.2e -> %.2e" % (rep["final_cost"], sum(cost_t), np.abs(b0).max(), np.abs(b1).max()))
    assert rep["final_cost"] <= sum(cost_t)
    assert np.abs(b1).max() < 1e-6 * np.abs(b0).max()


# ---- 6. noise reduction where it must occur ----
def test_static_object_noise_is_pooled():
    # the restatement alone (tests/test_smooth_restated_host.py): ratio 0.123 with this seed; expected 1/8 (64 frames pooled)
    ds, x0, zt = sc.static_object()
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, rep, _, _ = p.track_smooth(xt, 1e-5, 1e-5)
    a, b = sc.pose_rms(xs, ds, zt), sc.pose_rms(xt, ds, zt)
    print("static object: rms smooth %.3e, track %.3e, ratio %.3f" % (a, b, a / b), rep)
    assert a <= 0.5 * b, (a, b)


# ---- 7. contract ----
def test_two_calls_give_the_same_bits_and_track_is_unaffected():
    ds, g = _golden_track("g_track_cfg2_huber")
    x0 = ds.x_full
    with _problem(ds, 10.0) as p:
        a = p.track_smooth(x0, SROT, STRANS)
        b = p.track_smooth(x0, SROT, STRANS)
        t1 = p.track(x0, aar.lm_default_params())
    with _problem(ds, 10.0) as p:
        t0 = p.track(x0, aar.lm_default_params())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for k in ("iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost", "final_prior_cost", "final_mu"):
        assert a[1][k] == b[1][k], k
    assert a[1]["iterations"] > 1 and a[1]["seconds"] > 0
    for u, v in zip(t0, t1):
        assert np.array_equal(u, v)


def test_unsupported_behind_a_communicator():
    ds, g = _golden_track("g_track_cfg2")
    x0 = ds.x_full
    world = 2
    group = aar.LocalGroup(world)
    out = [None] * world

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with aar.Problem(ds, comm=comm) as p:
                codes = []
                for call in (lambda: p.track_smooth(x0, SROT, STRANS), lambda: p.track_smooth_system(x0, SROT, STRANS, 1.0)):
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


def test_intrinsics_from_the_pose_vector():
    ds, g = _golden_track("g_track_cfg2")
    with aar.Problem(ds, intrinsics=True) as p:
        x0 = p.x_with_intrinsics(ds.x_full)
        n0 = sc.ns(ds)
        q = x0[n0 + 6 * ds.num_frames:].reshape(ds.num_cams, 9)
        q[:, 0] *= 1.01
        q[:, 1] += 3.0
        x, rep, fe, pe = p.track_smooth(x0, SROT, STRANS)
    td = tr.TrackData(ds, x0, intrinsics=True)
    r = sr.smooth_lm(sr.SmoothProblem(td, SROT, STRANS), td.z0)
    rk = sr.smooth_lm(sr.SmoothProblem(tr.TrackData(ds, ds.x_full), SROT, STRANS), td.z0)
    assert abs(r["err"] - rk["err"]) > 1e-2 * rk["err"]          # the perturbed K matters
    assert r["margin"] > 1e-9 and rep["iterations"] == r["iterations"]
    np.testing.assert_allclose(rep["final_cost"], r["err"], rtol=1e-10)
    F = ds.num_frames
    assert np.abs(x[n0:n0 + 6 * F].reshape(-1, 6) - r["z"]).max() < 1e-9 + 2 * r["slack"]
    assert np.array_equal(x[:n0], x0[:n0]) and np.array_equal(x[n0 + 6 * F:], x0[n0 + 6 * F:])


def test_mapper_track_smooth(tmp_path):
    exe = str(tmp_path / "smooth_mapper_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_mapper_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = dict(l.split(" = ") for l in run.stdout.splitlines() if " = " in l)
    ds = aar.synth(2)
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        xt, _, et = p.track(x0, aar.lm_default_params())
        xs, rep, fe, pe = p.track_smooth(xt, SROT, STRANS, frame_time=np.asarray(ds.frame_ids, dtype=np.float64))
    assert int(kv["frames"]) == ds.num_frames and int(kv["pairs"]) == ds.num_frames - 1
    np.testing.assert_allclose(float(kv["track_err"]), et.sum(), rtol=1e-9)
    assert int(kv["iterations"]) == rep["iterations"] and int(kv["stop_code"]) == rep["stop_code"]
    np.testing.assert_allclose(float(kv["final_cost"]), rep["final_cost"], rtol=1e-9)
    np.testing.assert_allclose([float(kv["sum_frame_err"]), float(kv["sum_pair_err"])], [fe.sum(), pe.sum()], rtol=1e-8)
    z = np.array([[float(v) for v in kv["z%d" % f].split()] for f in range(ds.num_frames)])
    # (the mapper carries its poses as 4x4 matrices between the two calls: the round trip costs a few ulps of the start)
    assert np.abs(z - xs[sc.ns(ds):].reshape(-1, 6)).max() < 1e-8


def test_find_solution_smooth_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    os.replace(os.path.join(folder, "initial.solution"), os.path.join(folder, "initial_tracking_only.solution"))
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    got = {}
    for flag in ([], ["-smooth", "0.05", "0.02"]):
        run = subprocess.run(base + flag, capture_output=True, text=True, timeout=300, env=dict(os.environ, AAR_DETERMINISTIC="1"))
        assert run.returncode == 0, run.stdout + run.stderr
        assert ("smooth: " in run.stdout) == bool(flag)
        got[bool(flag)] = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    n0 = sc.ns(got[True])
    # cameras and markers are the solve's (the mapper carries every pose through a 4x4 matrix and back between its calls: a few ulps of
    # entries of order 1, held to 1e-12); the frames have moved
    assert np.abs(got[True].x_full[:n0] - got[False].x_full[:n0]).max() < 1e-12
    assert np.abs(got[True].x_full[n0:] - got[False].x_full[n0:]).max() > 1e-6
    # refused with the usage message: without -tracking-only, with one sigma, with a non-positive one
    for bad in ([exe, folder, "0.05", "x", "-from-initial", "-smooth", "0.05", "0.02"], base + ["-smooth", "0.05"], base + ["-smooth", "0.05", "-1"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "smooth: " not in run.stdout, run.stdout
