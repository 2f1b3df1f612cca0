"""The live tracker's marginalised anchor and per-push covariance (the tail instance of k_live_push) against the
float64 restatement tests/live_marginal_restated.py, against numpy.linalg.inv, against aar_track_smooth, and its contract.  Needs a real MI355X.

Bars: those of tests/test_gpu_live_tracker.py for the pushes (equal iteration, rejected-try and stop codes, final cost rtol 1e-10, poses
1e-9 + 2 slack, every restated margin above 1e-9); the marginal's information matrix 1e-8 of its largest entry, its mean as a pose; the covariance
blocks 1e-7 of the largest entry (the bar of aar_problem_covariance), sigma2 rtol 1e-10.

Measured on an MI355X while writing this test: see DESIGN.md section 19.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import aar
import live_detection_cases as ld
import live_marginal_cases as mc
import live_marginal_restated as lm
import pose_metrics as pm
import smooth_cases as sc
import track_restated as tr
from conftest import PKG

pytestmark = pytest.mark.gpu

KINDS = ["counts", "huber", "far"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def tracker(c, **over):
    return aar.Tracker(c.sol, params=aar.lm_default_params(**c.lm), **dict(c.kw, **over))


def push(t, c, f):
    cam, mk, uv = mc.frame_obs(c.ds, f)
    return t.push(c.times[f], cam, mk, uv, pose_init=c.td.z0[f] if c.has_init[f] else None)


@functools.lru_cache(maxsize=None)
def device(kind, lag, anchor, covariance, smooth=True, first_empty=False):
    """every push of a case on the device: [(result, uncertainty record, window)]"""
    c = mc.case(kind, lag, smooth, first_empty)
    out = []
    with tracker(c, anchor=anchor, covariance=covariance) as t:
        for f in range(c.n):
            g = push(t, c, f)
            out.append((g, t.uncertainty(), t.window()))
    return out


def compare_push(c, f, g, r, win):
    """tests/test_gpu_live_tracker.py's comparison of one push"""
    print("%s push %d: W %d it %d/%d rej %d/%d exit %d/%d cost %.12g/%.12g margin %.2e slack %.2e" % (
        c.name, f, g["window_frames"], g["iterations"], r["iterations"], g["rejected_tries"], r["rejected"], g["stop_code"], r["exit"],
        g["final_cost"], r["err"], r["margin"], r["slack"]))
    assert r["margin"] > 1e-9, (f, r["margin"])
    assert g["frame_index"] == f and g["window_frames"] == r["window_frames"]
    assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
    np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-10, atol=1e-300)
    np.testing.assert_allclose([g["final_data_cost"], g["final_prior_cost"]], [r["data"], r["prior"]], rtol=1e-9, atol=1e-12)
    tol = 1e-9 + 2 * r["slack"]
    assert np.abs(g["pose"] - r["pose"]).max() < tol
    assert (g["lagged_pose"] is None) == (r["lagged_pose"] is None)
    if r["lagged_pose"] is not None:
        assert g["lagged_index"] == f - c.lag and np.abs(g["lagged_pose"] - r["lagged_pose"]).max() < tol
    assert win["n"] == r["window_frames"] and np.abs(win["poses"] - r["window"]).max() < tol
    assert (win["anchor_pose"] is None) == (r["anchor"] is None)            # the fixed anchor pose is still kept in marginal mode
    if r["anchor"] is not None:
        assert np.abs(win["anchor_pose"] - r["anchor"]).max() < tol
    Ef, Pe = r["problem"].costs(r["window"])
    np.testing.assert_allclose(win["frame_err"], Ef, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(win["pair_err"], Pe, rtol=1e-7, atol=1e-12)
    return tol


def compare_marginal(f, u, r, tol):
    assert u["has_marginal"] == r["has_marginal"] and u["marginal_index"] == r["marginal_index"] and u["marginal_dropped"] == r["dropped"]
    if r["has_marginal"]:
        Lr, mr = r["marginal"]
        dL = np.abs(u["marginal_info"] - Lr).max() / np.abs(Lr).max()
        dm = np.abs(u["marginal_mean"] - mr).max()
        print("    marginal after push %d: info %.2e of its largest entry, mean %.2e" % (f, dL, dm))
        assert dL <= 1e-8 and dm < tol
        return dL
    return 0.0


# ---- 1. every push against the restated push, marginal mode ----
@pytest.mark.parametrize("lag", [1, 3, 15])
@pytest.mark.parametrize("kind", KINDS)
def test_every_push_against_the_restated_push(kind, lag):
    c, ref, dev = mc.case(kind, lag), mc.restated(kind, lag, "marginal"), device(kind, lag, "marginal", False)
    worst = 0.0
    for f in range(c.n):
        g, u, win = dev[f]
        tol = compare_push(c, f, g, ref[f], win)
        worst = max(worst, compare_marginal(f, u, ref[f], tol))
        assert u["cov_valid"] == 0 and not u["cov"].any() and u["sigma2"] == 0.0 and u["marginal_dropped"] == 0
        assert list(u["frame_index"]) == list(win["frame_index"])
    print("%s: largest marginal information difference %.2e" % (c.name, worst))
    assert [u["has_marginal"] for _, u, _ in dev] == [int(f >= lag) for f in range(c.n)]
    cnt = np.bincount(c.ds.obs_frame, minlength=c.n)
    if kind == "counts":
        assert 0 in cnt[1:-1] and 1 in cnt[1:-1]
        slots = lag + 1
        if slots < 8:
            assert any(cnt[f] < cnt[f - slots] for f in range(slots, c.n)) and any(cnt[f] > cnt[f - slots] for f in range(slots, c.n))
    if kind == "far":
        assert sum(r["rejected"] for r in ref) > 0


# ---- 2. the covariance blocks against numpy.linalg.inv of the restated H at the device's final poses ----
COV_CASES = [("fixed", 0, False), ("fixed", 0, True), ("fixed", 1, True), ("fixed", 3, True), ("fixed", 15, True),
             ("marginal", 1, True), ("marginal", 3, True), ("marginal", 15, True)]


@pytest.mark.parametrize("anchor,lag,smooth", COV_CASES, ids=["%s-lag%d-smooth%d" % (a, l, s) for a, l, s in COV_CASES])
def test_covariance_blocks_against_numpy_inv(anchor, lag, smooth):
    c, ref, dev = mc.case("counts", lag, smooth), mc.restated("counts", lag, anchor, smooth), device("counts", lag, anchor, True, smooth)
    worst, invalid = 0.0, 0
    for f in range(c.n):
        g, u, win = dev[f]
        r = ref[f]
        compare_push(c, f, g, r, win)
        cov, valid = lm.cov_blocks(r["problem"], win["poses"])
        assert u["cov_valid"] == int(valid) and u["window_frames"] == win["n"] and u["cov"].shape == (win["n"], 6, 6)
        if not valid:
            invalid += 1
            assert not u["cov"].any()
        else:
            d = np.abs(u["cov"] - cov).max() / np.abs(cov).max()
            worst = max(worst, d)
            assert d <= 1e-7, (f, d)
            assert np.array_equal(u["cov"], np.swapaxes(u["cov"], 1, 2))
        np.testing.assert_allclose(u["sigma2"], r["sigma2"], rtol=1e-10, atol=0.0)
    print("%s lag %d smooth %d: largest covariance difference %.3e of the largest entry, %d pushes without a covariance" % (
        anchor, lag, smooth, worst, invalid))
    cnt = np.bincount(c.ds.obs_frame, minlength=c.n)
    assert invalid == (int(np.sum(cnt == 0)) if not smooth else 0)          # smooth = 0 on an empty frame: cov_valid == 0


# ---- 3. covariance changes no bit of the push ----
def _bits(g, win):
    return [g[k] for k in ("iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost", "final_prior_cost",
                           "final_mu")] + list(g["pose"]) + ([] if g["lagged_pose"] is None else list(g["lagged_pose"])) + \
        list(win["poses"].reshape(-1)) + list(win["frame_err"]) + list(win["pair_err"])


def _ubits(u):
    return [u[k] for k in ("cov_valid", "sigma2", "window_frames", "has_marginal", "marginal_index", "marginal_dropped")] + \
        list(u["frame_index"]) + list(u["cov"].reshape(-1)) + list(u["marginal_info"].reshape(-1)) + list(u["marginal_mean"])


@pytest.mark.parametrize("anchor", ["fixed", "marginal"])
def test_covariance_changes_no_bit_of_the_push(anchor):
    c = mc.case("counts", 3)
    with_cov = device("counts", 3, anchor, True)
    if anchor == "marginal":
        without = [(g, w) for g, _, w in device("counts", 3, "marginal", False)]
    else:
        without = []
        with tracker(c) as t:                                               # both options off: the kernel of section 17
            with pytest.raises(aar.AarError) as e:
                t.uncertainty()
            assert e.value.code == aar.AAR_ERR_INVALID
            for f in range(c.n):
                g = push(t, c, f)
                without.append((g, t.window()))
            with pytest.raises(aar.AarError) as e:
                t.uncertainty()
            assert e.value.code == aar.AAR_ERR_INVALID and "covariance" in str(e.value)
    for f in range(c.n):
        assert _bits(with_cov[f][0], with_cov[f][2]) == _bits(*without[f]), f
    if anchor == "marginal":                                                # ... nor of the marginal
        for (_, ua, _), (_, ub, _) in zip(with_cov, device("counts", 3, "marginal", False)):
            assert np.array_equal(ua["marginal_info"], ub["marginal_info"]) and np.array_equal(ua["marginal_mean"], ub["marginal_mean"])


# ---- 4. reproducibility, reset, rejected pushes ----
def test_same_pushes_same_bits_reset_and_rejected_pushes():
    c = mc.case("counts", 3)
    first = device("counts", 3, "marginal", True)
    want = [_bits(g, w) + _ubits(u) for g, u, w in first]
    cam, mk, uv = mc.frame_obs(c.ds, 2)
    with tracker(c, anchor="marginal", covariance=True) as t:
        with pytest.raises(aar.AarError) as e:                              # before any push
            t.uncertainty()
        assert e.value.code == aar.AAR_ERR_INVALID
        for rnd in range(2):
            got = []
            for f in range(c.n):
                if f in (1, 5, 9):                                          # rejected pushes leave the record and the marginal untouched
                    before = _ubits(t.uncertainty())
                    for bad in (lambda: t.push(c.times[f], np.r_[cam[:-1], c.ds.num_cams], mk, uv, c.td.z0[f]),
                                lambda: t.push(c.times[f - 1], cam, mk, uv, c.td.z0[f])):
                        with pytest.raises(aar.AarError) as e:
                            bad()
                        assert e.value.code == aar.AAR_ERR_INVALID
                    assert _ubits(t.uncertainty()) == before
                g = push(t, c, f)
                got.append(_bits(g, t.window()) + _ubits(t.uncertainty()))
            assert got == want, rnd
            assert t.uncertainty()["has_marginal"] == 1
            t.reset()
            with pytest.raises(aar.AarError) as e:                          # reset clears the record and the marginal
                t.uncertainty()
            assert e.value.code == aar.AAR_ERR_INVALID
        g = push(t, c, 0)
        assert t.uncertainty()["has_marginal"] == 0 and t.uncertainty()["marginal_dropped"] == 0


# ---- 5. a stream that starts with an empty frame ----
def test_empty_stream_start_on_the_device():
    c, ref, dev = mc.case("plain", 3, True, True), mc.restated("plain", 3, "marginal", True, True), device("plain", 3, "marginal", True, True, True)
    for f in range(c.n):
        g, u, win = dev[f]
        tol = compare_push(c, f, g, ref[f], win)
        compare_marginal(f, u, ref[f], tol)
        assert np.isfinite(g["pose"]).all() and np.isfinite(u["cov"]).all()
    assert [u["marginal_dropped"] for _, u, _ in dev] == [0, 0, 0] + [1] * (c.n - 3)
    assert [u["has_marginal"] for _, u, _ in dev] == [0, 0, 0, 0] + [1] * (c.n - 4)


# ---- 6. the batch property ----
def _stream(ds, x0, lag, srot, strans, anchor, lm_params=None):
    """(newest poses [F, 6], lagged poses [F, 6] with the flushed window at the end, results)"""
    n0, F = sc.ns(ds), ds.num_frames
    newest, lagged, res = np.zeros((F, 6)), np.zeros((F, 6)), []
    with aar.Tracker(sc.copy_of(ds, x_full=x0), lag=lag, smooth=True, sigma_rot=srot, sigma_trans=strans, anchor=anchor, params=lm_params,
                     max_obs_per_frame=int(np.bincount(ds.obs_frame).max())) as t:
        for f in range(F):
            g = t.push(float(f), *mc.frame_obs(ds, f), pose_init=x0[n0:n0 + 6] if f == 0 else None)
            newest[f] = g["pose"]
            if g["has_lagged"]:
                lagged[g["lagged_index"]] = g["lagged_pose"]
            res.append(g)
        win = t.window()
        lagged[win["frame_index"]] = win["poses"]
    return newest, lagged, res


def test_marginal_anchor_is_closer_to_track_smooth():
    ds, x0 = mc.moving_object()
    n0, F, lag = sc.ns(ds), ds.num_frames, mc.BATCH_LAG
    prm = aar.lm_default_params(min_average_step_error_diff=1e-12)
    worst = {}
    batch = {}
    for anchor in ("fixed", "marginal"):
        _, _, res = _stream(ds, x0, lag, mc.BATCH_SROT, mc.BATCH_STRANS, anchor, prm)
        w = 0.0
        for f in range(lag, F):
            if f not in batch:
                keep = np.asarray(ds.obs_frame) <= f
                sub = sc.copy_of(ds, num_frames=f + 1, frame_ids=ds.frame_ids[:f + 1], obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep],
                                 obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep], x_full=x0[:n0 + 6 * (f + 1)])
                with aar.Problem(sub) as p:
                    xs = p.track_smooth(sub.x_full, mc.BATCH_SROT, mc.BATCH_STRANS, frame_time=np.arange(f + 1.0), params=prm)[0]
                batch[f] = xs[n0:].reshape(-1, 6)
            one = sc.copy_of(ds, num_frames=1)
            w = max(w, max(pm.pose_delta(one, np.r_[x0[:n0], res[f]["lagged_pose"]], np.r_[x0[:n0], batch[f][f - lag]])["frames"]))
        worst[anchor] = w
    print("batch property (device, 24 frames, lag 3): fixed %.3e, marginal %.3e" % (worst["fixed"], worst["marginal"]))
    assert worst["marginal"] < worst["fixed"]


# ---- 7. a static object ----
def test_static_object_marginal_lagged_poses_are_no_worse():
    ds, x0, zt = sc.static_object()
    n0 = sc.ns(ds)
    rms = {}
    for anchor in ("fixed", "marginal"):
        newest, lagged, _ = _stream(ds, x0, 3, 1e-5, 1e-5, anchor)
        rms[anchor] = (sc.pose_rms(np.r_[x0[:n0], newest.reshape(-1)], ds, zt), sc.pose_rms(np.r_[x0[:n0], lagged.reshape(-1)], ds, zt))
    print("static object, 64 frames, lag 3: newest rms fixed %.3e marginal %.3e (ratio %.3f); lagged rms fixed %.3e marginal %.3e (ratio %.3f)" % (
        rms["fixed"][0], rms["marginal"][0], rms["marginal"][0] / rms["fixed"][0], rms["fixed"][1], rms["marginal"][1],
        rms["marginal"][1] / rms["fixed"][1]))
    assert rms["marginal"][1] <= rms["fixed"][1]


# ---- 8. pushes of raw detections with both options ----
def test_push_detections_with_both_options():
    """aar_tracker_push_detections against aar_tracker_push fed the undistorted corners and the same start, on the DISTORTED scene.  The
    undistorted corners are the Initializer's (the same undistortion on the device, as tests/test_gpu_live_detections.py's alternating test
    takes them), so the two trackers see the same floats: poses are held to 1e-12 and the records to 1e-9 of their largest entry -- what is
    left is the order of the records' arithmetic, not the corners."""
    c = ld.case(True)
    out = aar.initializer_run(c.det, c.K, c.dists, c.ms, solution=c.sol)
    kw = dict(lag=2, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, anchor="marginal", covariance=True, max_obs_per_frame=64)
    worst = 0.0
    with aar.Tracker(c.sol, **kw) as ta, aar.Tracker(c.sol, **kw) as tb:
        ta.enable_detections(Ks=c.K, dists=c.dists)
        for f, (cam, mk, raw) in enumerate(c.frames):
            sel = np.asarray(out.obs_frame) == f
            np.testing.assert_array_equal(out.obs_cam[sel], cam)
            ga, info = ta.push_detections(float(f), cam, mk, raw)
            gb = tb.push(float(f), cam, mk, out.obs_uv[sel], pose_init=info["start_pose"])
            ua, ub = ta.uncertainty(), tb.uncertainty()
            assert (ga["iterations"], ga["rejected_tries"], ga["stop_code"]) == (gb["iterations"], gb["rejected_tries"], gb["stop_code"])
            assert np.abs(ga["pose"] - gb["pose"]).max() < 1e-12
            for k in ("cov_valid", "window_frames", "has_marginal", "marginal_index", "marginal_dropped"):
                assert ua[k] == ub[k], (f, k)
            dc = np.abs(ua["cov"] - ub["cov"]).max() / np.abs(ub["cov"]).max()
            worst = max(worst, dc)
            assert ua["cov_valid"] == 1 and dc <= 1e-9
            np.testing.assert_allclose(ua["sigma2"], ub["sigma2"], rtol=1e-9)
            if ub["has_marginal"]:
                dl = np.abs(ua["marginal_info"] - ub["marginal_info"]).max() / np.abs(ub["marginal_info"]).max()
                worst = max(worst, dl)
                assert dl <= 1e-9 and np.abs(ua["marginal_mean"] - ub["marginal_mean"]).max() < 1e-12
        assert ua["has_marginal"] == 1
    print("push_detections against push: largest record difference %.3e of the largest entry" % worst)


# ---- 9. the driver and the C++ mirror (MultiCamMapper::track_live -> aar::LiveTracker::uncertainty) ----
def parse_live_cov_yaml(path):
    """{frame id: (sigma2, scaled 6x6)} of aar_tracker_covariance_write_yaml's file"""
    txt = open(path).read()
    assert txt.startswith("%YAML:1.0\n---\nobject_poses:\n")
    num = lambda v: float(v.replace(".nan", "nan").replace(".inf", "inf"))
    blocks = {}
    for m in re.finditer(r"- \{ frame_id:(-?\d+), sigma_rot: (\S+), sigma_trans: (\S+),\s*covariance: !!opencv-matrix \{ rows:6, cols:6, dt:d, data:\[([^\]]*)\] \} \}",
                         txt):
        blk = np.array([num(v) for v in m.group(4).replace("\n", " ").split(",")]).reshape(6, 6)
        np.testing.assert_allclose([num(m.group(2)), num(m.group(3))], [np.sqrt(np.trace(blk[:3, :3]) / 3), np.sqrt(np.trace(blk[3:, 3:]) / 3)], rtol=1e-6)
        blocks[int(m.group(1))] = blk
    s2 = {int(m.group(1)): num(m.group(2)) for m in re.finditer(r"- \{ frame_id:(-?\d+), sigma2: (\S+) \}", txt)}
    assert set(s2) == set(blocks)
    return {k: (s2[k], blocks[k]) for k in blocks}


def test_find_solution_anchor_and_live_covariance_switches(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    ds = aar.solution_read(os.path.join(folder, "initial.solution"))
    os.replace(os.path.join(folder, "initial.solution"), os.path.join(folder, "initial_tracking_only.solution"))
    lag = 3
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    run = subprocess.run(base + ["-live", str(lag), repr(mc.SROT), repr(mc.STRANS), "-anchor", "marginal", "-live-covariance"], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0 and "live: " in run.stdout and "live covariance: " in run.stdout, run.stdout + run.stderr
    y = parse_live_cov_yaml(os.path.join(folder, "final_tracking_only.solution.covariance.yaml"))
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    n0, F = sc.ns(ds), ds.num_frames
    z, cov, s2 = np.zeros((F, 6)), np.zeros((F, 6, 6)), np.zeros(F)
    with aar.Tracker(ds, lag=lag, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, anchor="marginal", covariance=True,
                     max_obs_per_frame=int(np.bincount(ds.obs_frame).max())) as t:
        for f in range(F):
            t.push(float(ds.frame_ids[f]), *mc.frame_obs(ds, f), pose_init=ds.x_full[n0 + 6 * f: n0 + 6 * f + 6])
            u = t.uncertainty()
            assert u["cov_valid"] == 1
            cov[u["frame_index"]], s2[u["frame_index"]] = u["cov"], u["sigma2"]     # a frame keeps the last push it was in the window of
            win = t.window()
            z[win["frame_index"]] = win["poses"]
        assert u["has_marginal"] == 1 and u["marginal_dropped"] == 0
    assert sorted(y) == sorted(int(i) for i in ds.frame_ids)
    for f in range(F):
        sig, blk = y[int(ds.frame_ids[f])]
        np.testing.assert_allclose(sig, s2[f], rtol=1e-6)
        assert np.abs(blk - s2[f] * cov[f]).max() <= 1e-6 * np.abs(s2[f] * cov[f]).max(), f
    zf = got.x_full[n0:].reshape(-1, 6)
    assert np.abs(tr.rodrigues(zf[:, :3]) - tr.rodrigues(z[:, :3])).max() < 1e-8 and np.abs(zf[:, 3:] - z[:, 3:]).max() < 1e-8
    # -anchor marginal moves the poses; without -live-covariance no file is written; refused with the usage message: marginal without the
    # sigmas or with lag 0, an unknown anchor, the switches without -live
    os.remove(os.path.join(folder, "final_tracking_only.solution.covariance.yaml"))
    run = subprocess.run(base + ["-live", str(lag), repr(mc.SROT), repr(mc.STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not os.path.exists(os.path.join(folder, "final_tracking_only.solution.covariance.yaml"))
    fixed = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    assert np.abs(fixed.x_full[n0:] - got.x_full[n0:]).max() > 1e-9
    for bad in (base + ["-live", "0", "-anchor", "marginal"], base + ["-live", "0", repr(mc.SROT), repr(mc.STRANS), "-anchor", "marginal"],
                base + ["-live", "3", repr(mc.SROT), repr(mc.STRANS), "-anchor", "floating"], base + ["-live-covariance"],
                base + ["-live", "3", repr(mc.SROT), repr(mc.STRANS), "-anchor"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "live: " not in run.stdout, run.stdout
