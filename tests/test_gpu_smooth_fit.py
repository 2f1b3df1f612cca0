"""Fitting the smoother's noise levels (aar_track_smooth_fit, aar_track_smooth_fit_terms) against the float64 restatement
tests/smooth_fit_restated.py (numpy.linalg.inv of the dense H, the between factor's Jacobian by complex step).  Needs a real MI355X.

Bars: the pairs' terms and their sums 10 eps kappa_2(H) relative to the reference value (the bar DESIGN.md section 28 holds the blocks to that
the terms are built from); the path of a fixed-length run 1e-8 relative (the project's bar for a direct solve against solveh_banded) with equal
LM step counts; recovery within smooth_fit_cases.CAPS.

tests/golden/smooth_fit_parent.npz holds aar_track_smooth's and aar_track_smooth_covariance's outputs on the three cases of
smooth_fit_cases.parent_cases(), recorded on an MI355X at the commit before their bodies moved into functions the fit shares:
    PYTHONPATH=automatic-ar_amd:tests python -c "import smooth_fit_cases as c; c.parent_write('tests/golden/smooth_fit_parent.npz')"
(two recordings were bit-equal).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import aar
import rotation_edge_cases as rec
import smooth_cases as sc
import smooth_fit_cases as fc
import smooth_fit_restated as fr
import track_restated as tr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SROT, STRANS = fc.SROT, fc.STRANS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _kappa(H):
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    return float(ev[-1] / ev[0])


# ---- 1. the terms against the restatement, 2. sanity of the sums ----
@functools.lru_cache(maxsize=None)
def _terms_case(F):
    """emptied frames (from 30 frames on), a frame_time hole every seventh pair, rel_motion on every pair, and from three frames on one pair
    whose expected motion leaves a residual rotation of 3 rad"""
    ds = fc.shape_dataset(F)
    x0 = sc.track_start(ds)
    ft = fc.gaps(F)
    rel = fc.rel_motion(F)
    if F >= 3:
        z = x0[sc.ns(ds): sc.ns(ds) + 6 * F].reshape(F, 6)
        k = F // 2
        rel[k] = rec.between_rel(z[k], z[k + 1], 3.0, rec.AXES[9], np.random.default_rng(11))
    return ds, x0, ft, rel


@pytest.mark.parametrize("F", [2, 3, 64, 65, 257, 513])
def test_terms_against_the_restatement(F):
    ds, x0, ft, rel = _terms_case(F)
    td = tr.TrackData(ds, x0)
    e = fr.estep(fr.FitProblem(td, ft, rel), td.z0, SROT, STRANS)
    kappa = _kappa(e["H"])
    bar = 10 * EPS * kappa
    with aar.Problem(ds) as p:
        terms, sums = p.track_smooth_fit_terms(x0, SROT, STRANS, frame_time=ft, rel_motion=rel)
    assert terms.shape == (F - 1, 4)
    if F >= 3:
        assert abs(np.sqrt(e["terms"][F // 2, 0] * np.diff(ft)[F // 2]) - 3.0) < 1e-6      # the 3 rad pair is in
    e_t = float(np.max(np.abs(terms - e["terms"]) / np.abs(e["terms"])))
    e_s = float(np.max(np.abs(sums - e["sums"]) / np.abs(e["sums"])))
    print("F %d: kappa %.3e, pair terms %.2e sums %.2e = %.4f / %.4f eps kappa" % (F, kappa, e_t, e_s, e_t / (EPS * kappa), e_s / (EPS * kappa)))
    assert e_t <= bar and e_s <= bar, (e_t, e_s, bar)
    # sanity of the sums: the prior's share of tr(H H^-1) = 6 F lies strictly between nothing and all of it
    share = sums[1] / SROT ** 2 + sums[3] / STRANS ** 2
    assert 0 < share < 6 * F, (share, 6 * F)
    assert np.all(terms > 0)


# ---- 3. a fixed-length run against the restated loop ----
@functools.lru_cache(maxsize=None)
def _loop_case(name):
    if name == "walk48":
        ds, x0 = fc.random_walk(48, *fc.WALK_SIGMAS, seed=5)
        return ds, x0, None, None
    ds = fc.shape_dataset(65)
    return ds, sc.track_start(ds), fc.gaps(65), None


@pytest.mark.parametrize("name", ["walk48", "emptied65_gaps"])
def test_fixed_length_run_against_the_restated_loop(name):
    ds, x0, ft, rel = _loop_case(name)
    td = tr.TrackData(ds, x0)
    r = fr.fit(fr.FitProblem(td, ft, rel), td.z0, SROT, STRANS, max_iters=5, rel_tol=0.0)
    assert r["margin"] > 1e-9 and r["iterations"] == 5 and r["stop_code"] == 2        # no LM decision of the restated runs is a toss-up
    with aar.Problem(ds) as p:
        x, rep, path = p.track_smooth_fit(x0, SROT, STRANS, frame_time=ft, rel_motion=rel, fit=dict(max_iters=5, rel_tol=0.0))
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
    assert np.array_equal(x[:n0], x0[:n0]) and np.abs(x[n0:n0 + 6 * td.F].reshape(-1, 6) - r["z"]).max() < 1e-7
    assert rep["launches"] > 0 and rep["seconds"] > 0


# ---- 4. fixed point, 5. recovery, 6. two identical calls ----
@functools.lru_cache(maxsize=None)
def _device_fit(seed):
    ds, x0 = fc.walk(seed)
    with aar.Problem(ds) as p:
        a = p.track_smooth_fit(x0, SROT, STRANS)
        b = p.track_smooth_fit(x0, SROT, STRANS)
        x, rep, _ = a
        terms, sums = p.track_smooth_fit_terms(x, rep["sigma_rot_eff"], rep["sigma_trans_eff"])
        cost = p.track_smooth_system(x, rep["sigma_rot_eff"], rep["sigma_trans_eff"], 0.0)[4]
    return ds, a, b, sums, cost


def test_recovery_on_the_device():
    ds, (x, rep, path), _, _, _ = _device_fit(100)
    dev = np.array([rep["sigma_px"], rep["sigma_rot"], rep["sigma_trans"]]) / fc.WALK_SIGMAS - 1.0
    print("seed 100: %d EM iterations (exit %d, %d LM steps, %d launches, %.3f s), deviations %s" %
          (rep["iterations"], rep["stop_code"], rep["lm_steps"], rep["launches"], rep["seconds"], np.array2string(dev, precision=5)))
    assert rep["stop_code"] == 1 and rep["iterations"] < 50 and rep["last_rel_change"] < 1e-3
    assert np.all(np.abs(dev) <= fc.CAPS), (dev, fc.CAPS)


def test_fixed_point():
    ds, (x, rep, path), _, sums, cost = _device_fit(100)
    F, N = ds.num_frames, ds.num_obs
    q, s_r, s_t = rep["sigma_px"] ** 2, rep["sigma_rot"] ** 2, rep["sigma_trans"] ** 2
    U_d = 6.0 * F - sums[1] / rep["sigma_rot_eff"] ** 2 - sums[3] / rep["sigma_trans_eff"] ** 2
    new = fr.mstep(sums, cost[0], U_d, q, s_r, s_t, F, N)
    move = max(abs(np.sqrt(a) / np.sqrt(b) - 1.0) for a, b in zip(new, (q, s_r, s_t)))
    print("one more M-step at the reported values moves a sigma by at most %.2e" % move)
    assert move <= 1e-3, move


def test_two_identical_calls():
    _, (xa, ra, pa), (xb, rb, pb), _, _ = _device_fit(100)
    assert np.array_equal(xa, xb) and np.array_equal(pa, pb)
    for k in ra:
        assert k == "seconds" or ra[k] == rb[k], k


# ---- 7. estimate_px = 0 ----
def test_effective_sigmas_alone():
    ds, x0, ft, _ = _loop_case("emptied65_gaps")
    with aar.Problem(ds) as p:
        x, rep, path = p.track_smooth_fit(x0, SROT, STRANS, frame_time=ft, fit=dict(estimate_px=0, max_iters=8))
        y, rep2, path2 = p.track_smooth_fit(x0, SROT, STRANS, frame_time=ft, fit=dict(estimate_px=0, estimate_trans=0, max_iters=8))
    assert rep["sigma_px"] == 1.0 and np.all(path[:, 0] == 1.0)
    assert rep["sigma_rot_eff"] == rep["sigma_rot"] and rep["sigma_trans_eff"] == rep["sigma_trans"]
    assert rep["sigma_rot"] != SROT and rep["sigma_trans"] != STRANS
    np.testing.assert_allclose(path2[:, 2], STRANS, rtol=1e-15)                  # a sigma held fixed stays at its start value
    assert rep2["sigma_px"] == 1.0 and rep2["sigma_rot"] != SROT


# ---- 8. refusals ----
def _code(fn):
    with pytest.raises(aar.AarError) as e:
        fn()
    return e.value.code, str(e.value)


def test_refusals():
    ds = aar.synth(2, num_frames=6)
    x0 = sc.track_start(ds)
    with aar.Problem(ds, with_huber=True) as p:
        for fn in (lambda: p.track_smooth_fit(x0, SROT, STRANS), lambda: p.track_smooth_fit_terms(x0, SROT, STRANS)):
            code, msg = _code(fn)
            assert code == aar.AAR_ERR_UNSUPPORTED and "Huber" in msg and "Gaussian" in msg, msg
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            for fn in (lambda: p.track_smooth_fit(x0, SROT, STRANS), lambda: p.track_smooth_fit_terms(x0, SROT, STRANS)):
                code, msg = _code(fn)
                assert code == aar.AAR_ERR_UNSUPPORTED and "single-GPU only" in msg, msg
    finally:
        comm.close()
        group.close()
    one = aar.synth(2, num_frames=1)
    with aar.Problem(one) as p:
        for fn in (lambda: p.track_smooth_fit(sc.track_start(one), SROT, STRANS), lambda: p.track_smooth_fit_terms(sc.track_start(one), SROT, STRANS)):
            code, msg = _code(fn)
            assert code == aar.AAR_ERR_INVALID and "num_frames" in msg, msg
    none = sc.without_frames(ds, range(6))
    assert none.num_obs == 0
    with aar.Problem(none) as p:
        for fn in (lambda: p.track_smooth_fit(x0, SROT, STRANS), lambda: p.track_smooth_fit_terms(x0, SROT, STRANS)):
            code, msg = _code(fn)
            assert code == aar.AAR_ERR_INVALID and "no detections" in msg, msg
    with aar.Problem(ds) as p:
        keep = np.array(x0)
        for bad, word in ((dict(estimate_px=0, estimate_rot=0, estimate_trans=0), "estimate"), (dict(rel_tol=-1.0), "rel_tol"),
                          (dict(rel_tol=float("nan")), "rel_tol"), (dict(max_iters=0), "max_iters")):
            code, msg = _code(lambda: p.track_smooth_fit(x0, SROT, STRANS, fit=bad))
            assert code == aar.AAR_ERR_INVALID and word in msg, msg
        code, _ = _code(lambda: p.track_smooth_fit(x0, -1.0, STRANS))
        assert code == aar.AAR_ERR_INVALID and np.array_equal(x0, keep)
        # NULL fit parameters, path and report
        x = np.array(p._x(x0), dtype=np.float64)
        sp = aar.SmoothParams(SROT, STRANS)
        assert aar.lib().aar_track_smooth_fit(p.handle, aar._dptr(x), None, C.byref(sp.c), None, None, None) == 0
        assert np.array_equal(x, p.track_smooth_fit(x0, SROT, STRANS)[0])


# ---- 9. the refactor changed nothing ----
@pytest.mark.parametrize("which", [0, 1, 2])
def test_smoothing_and_covariance_keep_the_parent_commits_bits(which):
    g = np.load(os.path.join(ROOT, "tests", "golden", "smooth_fit_parent.npz"))
    name, ds, x0, ft, rel = fc.parent_cases()[which]
    with aar.Problem(ds) as p:
        got = fc.parent_record(p, x0, ft, rel)
    assert sorted(k for k in g.files if k.startswith(name + ".")) == sorted("%s.%s" % (name, k) for k in got)
    for k, v in got.items():
        assert np.array_equal(v, g["%s.%s" % (name, k)]), (name, k)


# ---- 10. the C++ mirror and the driver ----
def _kv(stdout):
    return dict(l.split(" = ") for l in stdout.splitlines() if " = " in l)


def test_mapper_fit_smooth_sigmas(tmp_path):
    exe = str(tmp_path / "smooth_fit_mapper_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_fit_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                         "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = _kv(run.stdout)
    ds = aar.synth(2)
    F = ds.num_frames
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, rep, path = p.track_smooth_fit(xt, SROT, STRANS, frame_time=np.asarray(ds.frame_ids, dtype=np.float64))
    assert int(kv["iterations"]) == rep["iterations"] and int(kv["stop_code"]) == rep["stop_code"] and int(kv["rows"]) == rep["iterations"] + 1
    # (the mapper carries its poses as 4x4 matrices between its calls: a few ulps of the start, 1e-8 in the poses as tests/test_gpu_track_smooth.py
    # holds them; the sigmas follow the track)
    for k in ("sigma_px", "sigma_rot", "sigma_trans", "sigma_rot_eff", "sigma_trans_eff"):
        np.testing.assert_allclose(float(kv[k]), rep[k], rtol=1e-6, err_msg=k)
    np.testing.assert_allclose(np.array([float(v) for v in kv["path"].split()]).reshape(-1, 3), path, rtol=1e-6)
    z = np.array([float(v) for v in kv["z"].split()]).reshape(F, 6)
    zs = xs[sc.ns(ds):sc.ns(ds) + 6 * F].reshape(F, 6)
    assert np.abs(z[:, 3:] - zs[:, 3:]).max() < 1e-6 and np.abs(tr.rodrigues(z[:, :3]) - tr.rodrigues(zs[:, :3])).max() < 1e-6


def test_find_solution_fit_sigmas_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # the first 90 frames, as tests/test_gpu_track_smooth_covariance.py cuts the recording: the later ones turn through pi, where the solution
    # file's vec -> matrix -> vec round trip lands on another rotation vector
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    env = dict(os.environ, AAR_DETERMINISTIC="1")
    # the solve alone, then the solve with the fit and the smoothing on top
    run = subprocess.run(base, capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "smooth-fit: " not in run.stdout, run.stdout + run.stderr
    solved = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    run = subprocess.run(base + ["-smooth", repr(SROT), repr(STRANS), "-fit-sigmas"], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("smooth-fit: ")]
    assert len(line) == 1 and "smooth: " in run.stdout, run.stdout
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    ft = np.asarray(solved.frame_ids, dtype=np.float64)
    with aar.Problem(solved) as p:
        xt, _, _ = p.track(solved.x_full, aar.lm_default_params())
        xf, rep, _ = p.track_smooth_fit(xt, SROT, STRANS, frame_time=ft)
        xs, _, _, _ = p.track_smooth(xf, rep["sigma_rot_eff"], rep["sigma_trans_eff"], frame_time=ft)
    words = line[0].split()
    for k in ("sigma_px", "sigma_rot", "sigma_trans", "sigma_rot_eff", "sigma_trans_eff"):
        np.testing.assert_allclose(float(words[words.index(k) + 1]), rep[k], rtol=1e-6, err_msg=k)
    assert int(words[words.index("after") + 1]) == rep["iterations"]
    assert np.abs(got.x_full - xs).max() < 1e-6
    assert np.abs(got.x_full[n0:] - solved.x_full[n0:]).max() > 1e-6
    # refused with the usage message: without -smooth, together with -live
    for bad in (base + ["-fit-sigmas"], base + ["-live", "0", "-fit-sigmas"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-fit-sigmas" in run.stdout and "smooth-fit: " not in run.stdout, run.stdout
