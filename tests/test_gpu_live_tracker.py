"""The live tracker (aar_tracker_*: one frame per push, fixed-lag smoothing, the whole LM of a push in one launch of k_live_push) against
the float64 restatement tests/live_restated.py, against aar_track / aar_track_smooth on the same frames, and its contract.  Needs a real MI355X.

Bars, those tests/test_gpu_track_smooth.py holds for the same quantities: equal iteration, rejected-try and stop codes, final cost rtol 1e-10,
poses 1e-9 + 2 slack; smooth = 0 against aar_track 1e-12.  Every push of every case is compared, and every push's restated margin must
exceed 1e-9.  (The lag-15 case has 3 * 16 + 1 = 49 pushes: the one more than 48 that lets every ring slot be used a third time and the first
one a fourth.)

Margins of the restated pushes (the smallest over the pushes of each case), measured on the CPU while writing this test:
    track (smooth 0) 3.0e-4, lag0 1.2e-3, lag1 2.1e-4, lag3 5.6e-5, lag15 5.3e-5, shrink 8.2e-4, special 2.7e-4, huber 4.2e-6,
    far 5.5e-4 (4 rejected tries, slack 2.2e-7; every other case has slack 0)
"""
import functools
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import aar
import live_restated as lr
import smooth_cases as sc
import track_restated as tr
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

SROT, STRANS = 0.05, 0.02      # as tests/test_gpu_track_smooth.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _times(n):
    """push times with a hole of five every seventh frame"""
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(n - 1) % 7 == 3) * 4.0])


def _keep_first(ds, counts):
    """the data set with only the first counts[f] detections of frame f (None: all)"""
    keep = np.ones(ds.num_obs, dtype=bool)
    for f, c in enumerate(counts):
        idx = np.nonzero(np.asarray(ds.obs_frame) == f)[0]
        if c is not None:
            keep[idx[c:]] = False
    return sc.copy_of(ds, obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep], obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep])


def frame_obs(ds, f):
    sel = np.asarray(ds.obs_frame) == f
    return ds.obs_cam[sel], ds.obs_marker[sel], ds.obs_uv[sel]


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of a case: data set, starts, push times, tracker and LM settings, and which pushes carry a pose_init"""
    lag, delta, lm, scale, smooth = 3, None, {}, 1.0, True
    every_init = False
    if name.startswith("lag"):
        lag = int(name[3:])
        n = 3 * (lag + 1) + 1
    elif name == "shrink":
        lag, n = 1, 16
    elif name == "special":
        n = 12
    elif name == "huber":
        n, delta = 13, 0.5
    elif name == "far":
        n, scale, lm, every_init = 24, 20.0, dict(tau=1e-6), True
    elif name == "track":
        lag, n, smooth, every_init = 0, 20, False, True
    else:
        raise KeyError(name)
    ds = aar.synth(2, num_frames=n, init_scale=scale)
    x0 = sc.track_start(ds)
    cnt = np.bincount(ds.obs_frame, minlength=n)
    if name == "shrink":
        # two ring slots; each slot's successive frames: full, fewer, fewer, ..., full again (the refill), fewer
        pattern = [4, 4, 3, 2, 5, 5, 3, 2, 5, 5, 2, 1, 1, 0, 0, 0]
        assert np.all(cnt >= pattern) and cnt.max() == 5
        ds = _keep_first(ds, pattern)
        assert list(np.bincount(ds.obs_frame, minlength=n)) == pattern
    if name == "special":
        ds = _keep_first(ds, [None, None, None, None, 0, None, 1, None, None, None, None, None])
        cam8 = ds.obs_cam[np.asarray(ds.obs_frame) == 8][0]
        keep = (np.asarray(ds.obs_frame) != 8) | (ds.obs_cam == cam8)       # frame 8: one camera only
        ds = sc.copy_of(ds, obs_frame=ds.obs_frame[keep], obs_cam=ds.obs_cam[keep], obs_marker=ds.obs_marker[keep], obs_uv=ds.obs_uv[keep])
    if name == "huber":
        uv = np.array(ds.obs_uv)
        rng = np.random.default_rng(11)
        hit = rng.choice(len(uv), size=len(uv) // 8, replace=False)
        uv[hit, rng.integers(0, 8, size=len(hit))] += 50.0                  # 50 px outliers
        ds = sc.copy_of(ds, obs_uv=uv.astype(np.float32))
    td = tr.TrackData(ds, x0)
    has_init = [True if every_init else (f % 3 != 1) for f in range(n)]
    kw = dict(lag=lag, smooth=smooth, with_huber=delta is not None, max_obs_per_frame=int(max(np.bincount(ds.obs_frame, minlength=n).max(), 1)))
    if smooth:
        kw.update(sigma_rot=SROT, sigma_trans=STRANS)
    if delta is not None:
        kw.update(huber_delta=delta)
    return SimpleNamespace(name=name, ds=ds, x0=x0, td=td, n=n, lag=lag, smooth=smooth, times=_times(n), delta=delta, lm=lm, kw=kw, has_init=has_init,
                           sol=sc.copy_of(ds, x_full=x0))


@functools.lru_cache(maxsize=None)
def restated(name):
    c = case(name)
    live = lr.Live(c.td, lag=c.lag, smooth=c.smooth, sigma_rot=SROT, sigma_trans=STRANS, delta=-1.0 if c.delta is None else c.delta, **c.lm)
    out = []
    for f in range(c.n):
        r = live.push(f, c.times[f], pose_init=c.td.z0[f] if c.has_init[f] else None)
        r["window"], r["anchor"] = live.window()
        out.append(r)
    return out


def tracker(c, **over):
    return aar.Tracker(c.sol, params=aar.lm_default_params(**c.lm), **dict(c.kw, **over))


def push(t, c, f):
    cam, mk, uv = frame_obs(c.ds, f)
    return t.push(c.times[f], cam, mk, uv, pose_init=c.td.z0[f] if c.has_init[f] else None)


def compare(c, f, g, r, win=None):
    """one push of the device (g, win = the window after it) against the restated push r"""
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
    assert (g["lagged_pose"] is None) == (r["lagged_pose"] is None) and bool(g["has_lagged"]) == (r["lagged_pose"] is not None)
    if r["lagged_pose"] is not None:
        assert g["lagged_index"] == f - c.lag and np.abs(g["lagged_pose"] - r["lagged_pose"]).max() < tol
    if win is not None:
        assert win["n"] == r["window_frames"] and list(win["frame_index"]) == list(range(f + 1 - win["n"], f + 1))
        assert np.abs(win["poses"] - r["window"]).max() < tol
        assert (win["anchor_pose"] is None) == (r["anchor"] is None)
        if r["anchor"] is not None:
            assert np.abs(win["anchor_pose"] - r["anchor"]).max() < tol
        Ef, Pe = r["problem"].costs(r["window"])
        np.testing.assert_allclose(win["frame_err"], Ef, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(win["pair_err"], Pe, rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(win["frame_err"].sum() + win["pair_err"].sum(), g["final_cost"], rtol=1e-12)


def run_against_restated(name, windows=True):
    c, ref = case(name), restated(name)
    out = []
    with tracker(c) as t:
        for f in range(c.n):
            g = push(t, c, f)
            compare(c, f, g, ref[f], t.window() if windows else None)
            out.append(g)
    return c, ref, out


# ---- 1. smooth = 0: k_track's loop, one frame per push ----
def test_smooth_0_is_track_frame_by_frame():
    c, ref = case("track"), restated("track")
    with aar.Problem(c.ds) as p:
        xt, it, et = p.track(c.x0, aar.lm_default_params())
    zt = xt[sc.ns(c.ds):].reshape(-1, 6)
    with tracker(c) as t:
        for f in range(c.n):
            g = push(t, c, f)
            assert g["iterations"] == it[f] and g["window_frames"] == 1 and g["final_prior_cost"] == 0.0
            assert np.abs(g["pose"] - zt[f]).max() < 1e-12
            np.testing.assert_allclose(g["final_cost"], et[f], rtol=1e-12)
            assert g["has_lagged"] and g["lagged_index"] == f and np.array_equal(g["lagged_pose"], g["pose"])
            r = ref[f]
            assert r["margin"] > 1e-9
            assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
            assert np.abs(g["pose"] - r["pose"]).max() < 1e-12 + 2 * r["slack"]
            np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-12)


# ---- 2. smooth = 1: every push against the restated push ----
@pytest.mark.parametrize("lag", [0, 1, 3, 15])
def test_every_push_against_the_restated_push(lag):
    c, ref, out = run_against_restated("lag%d" % lag)
    assert c.n >= 3 * (lag + 1) + 1                                         # every ring slot is reused
    assert [r["problem"].anchor is not None for r in ref] == [f > lag for f in range(c.n)]      # the fill phase, then every push anchored
    assert not all(c.has_init) and c.has_init[0]                            # both kinds of start occur


# ---- 3. the fill phase against aar_track_smooth ----
def test_fill_phase_is_track_smooth():
    c = case("lag3")
    n0 = sc.ns(c.ds)
    with tracker(c) as t:
        for k in range(c.lag + 1):
            before = t.window()["poses"] if k else np.zeros((0, 6))
            start = np.vstack([before, (c.td.z0[k] if c.has_init[k] else before[-1])[None, :]])
            g = push(t, c, k)
            win = t.window()
            sub = sc.without_frames(c.ds, range(k + 1, c.n))
            keep = np.asarray(sub.obs_frame) <= k
            sub = sc.copy_of(sub, num_frames=k + 1, frame_ids=sub.frame_ids[:k + 1], x_full=np.r_[c.x0[:n0], start.reshape(-1)])
            assert keep.all()
            with aar.Problem(sub) as p:
                xs, rep, fe, pe = p.track_smooth(sub.x_full, SROT, STRANS, frame_time=c.times[:k + 1])
            assert rep["iterations"] == g["iterations"] and rep["rejected_tries"] == g["rejected_tries"] and rep["stop_code"] == g["stop_code"]
            assert np.abs(win["poses"] - xs[n0:].reshape(-1, 6)).max() < 1e-10
            np.testing.assert_allclose(g["final_cost"], rep["final_cost"], rtol=1e-10)
            np.testing.assert_allclose(win["frame_err"], fe, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(win["pair_err"][1:], pe, rtol=1e-7, atol=1e-12)
            assert win["pair_err"][0] == 0.0 and win["anchor_pose"] is None


# ---- 4. ring reuse with shrinking frames ----
def test_ring_reuse_with_shrinking_frames():
    c, ref, out = run_against_restated("shrink")
    cnt = np.bincount(c.ds.obs_frame, minlength=c.n)
    assert cnt.max() == c.kw["max_obs_per_frame"]
    for f in range(2, c.n):
        assert cnt[f] <= cnt[f - 2] or cnt[f] == cnt.max()                  # a slot's next frame is smaller, or the refill after smaller ones
    assert sum(cnt[f] < cnt[f - 2] for f in range(2, c.n)) >= 8 and sum(cnt[f] > cnt[f - 2] for f in range(2, c.n)) >= 2


# ---- 5. special frames inside the window ----
def test_special_frames_inside_the_window():
    c, ref, out = run_against_restated("special")
    cnt = np.bincount(c.ds.obs_frame, minlength=c.n)
    assert cnt[4] == 0 and cnt[6] == 1 and len(set(c.ds.obs_cam[np.asarray(c.ds.obs_frame) == 8])) == 1 and cnt[8] > 1
    # the emptied frame moves with its neighbours: its final (lagged) pose is not where it started (the previous frame's estimate)
    assert not c.has_init[4]
    assert np.abs(out[4 + c.lag]["lagged_pose"] - out[3]["pose"]).max() > 1e-4
    # smooth = 0: it keeps its start bit for bit
    with tracker(c, lag=0, smooth=False, sigma_rot=0.0, sigma_trans=0.0) as t:
        cam, mk, uv = frame_obs(c.ds, 3)
        t.push(0.0, cam, mk, uv, pose_init=c.td.z0[3])
        cam, mk, uv = frame_obs(c.ds, 4)
        g = t.push(1.0, cam, mk, uv, pose_init=c.td.z0[4])
        assert g["iterations"] == 0 and np.array_equal(g["pose"], c.td.z0[4]) and g["final_cost"] == 0.0
        g2 = t.push(2.0, cam, mk, uv)                                       # ... also when the start is the previous frame's estimate
        assert g2["iterations"] == 0 and np.array_equal(g2["pose"], g["pose"])


# ---- 6. Huber ----
def test_huber_with_outliers():
    c, ref, out = run_against_restated("huber")
    assert sum(tr.weighted(r["problem"].fd[-1], r["pose"], c.delta)[1].sum() for r in ref) > 0      # corners past delta at the results


# ---- 7. far start ----
def test_far_start_with_rejected_tries():
    c, ref, out = run_against_restated("far")
    assert sum(r["rejected"] for r in ref) > 0 and [g["rejected_tries"] for g in out] == [r["rejected"] for r in ref]


# ---- 8. the anchor is final ----
def test_anchor_is_the_lagged_pose_bit_for_bit():
    c = case("lag3")
    with tracker(c) as t:
        prev = None
        seen = 0
        for f in range(c.n):
            g = push(t, c, f)
            win = t.window()
            if prev is not None:
                assert win["anchor_pose"] is not None and np.array_equal(win["anchor_pose"], prev)
                seen += 1
            else:
                assert win["anchor_pose"] is None
            prev = g["lagged_pose"]
            if prev is not None:
                assert np.array_equal(prev, win["poses"][0]) and g["lagged_index"] == win["frame_index"][0]
        assert seen == c.n - c.lag - 1


# ---- 9. reproducibility ----
def _bits(g):
    return [g[k] for k in ("iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost", "final_prior_cost", "final_mu")] + \
        list(g["pose"]) + ([] if g["lagged_pose"] is None else list(g["lagged_pose"]))


def test_two_trackers_and_a_reset_give_the_same_bits():
    c = case("lag3")
    with tracker(c) as a, tracker(c) as b:
        ra = [_bits(push(a, c, f)) for f in range(c.n)]
        rb = [_bits(push(b, c, f)) for f in range(c.n)]
        wa = a.window()
        a.reset()
        assert a.window()["n"] == 0
        rc = [_bits(push(a, c, f)) for f in range(c.n)]
        wc = a.window()
    assert ra == rb and ra == rc
    for k in ("poses", "frame_err", "pair_err", "anchor_pose"):
        assert np.array_equal(wa[k], wc[k])


# ---- 10. rejected pushes ----
def test_rejected_pushes_leave_the_tracker_as_it_was():
    c, ref = case("lag3"), restated("lag3")
    with tracker(c) as clean:
        want = [_bits(push(clean, c, f)) for f in range(6)]
    cam, mk, uv = frame_obs(c.ds, 2)
    nmax = c.kw["max_obs_per_frame"]

    def bad_pushes(t, f):
        tm = c.times[f]
        z = c.td.z0[f]
        big = nmax + 1
        tries = [("n_obs", lambda: t.push(tm, np.zeros(big, np.int32), np.zeros(big, np.int32), np.zeros((big, 8), np.float32), z)),
                 ("obs_cam", lambda: t.push(tm, np.r_[cam[:-1], c.ds.num_cams], mk, uv, z)),
                 ("obs_cam", lambda: t.push(tm, np.r_[cam[:-1], -1], mk, uv, z)),
                 ("obs_marker", lambda: t.push(tm, cam, np.r_[mk[:-1], c.ds.num_markers], uv, z)),
                 ("frame_time", lambda: t.push(np.nan, cam, mk, uv, z)),
                 ("frame_time", lambda: t.push(np.inf, cam, mk, uv, z)),
                 ("pose_init", lambda: t.push(tm, cam, mk, uv, np.r_[z[:5], np.nan]))]
        if f > 0:
            tries.append(("frame_time", lambda: t.push(c.times[f - 1], cam, mk, uv, z)))       # not above the previous one
        else:
            tries.append(("pose_init", lambda: t.push(tm, cam, mk, uv, None)))                  # the first push needs one
        for word, call in tries:
            with pytest.raises(aar.AarError) as e:
                call()
            assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), (word, str(e.value))

    with tracker(c) as t:
        got = []
        for f in range(6):
            bad_pushes(t, f)
            got.append(_bits(push(t, c, f)))
    assert got == want


# ---- 11. a static object: the lagged poses pool the noise ----
def test_static_object_lagged_poses_beat_track():
    ds, x0, zt = sc.static_object()
    n0 = sc.ns(ds)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
    z = np.zeros((ds.num_frames, 6))
    cam, mk, _ = frame_obs(ds, 0)
    with aar.Tracker(sc.copy_of(ds, x_full=x0), lag=15, smooth=True, sigma_rot=1e-5, sigma_trans=1e-5, max_obs_per_frame=len(cam)) as t:
        for f in range(ds.num_frames):
            g = t.push(float(f), *frame_obs(ds, f), pose_init=x0[n0:n0 + 6] if f == 0 else None)
            if g["has_lagged"]:
                z[g["lagged_index"]] = g["lagged_pose"]
        win = t.window()
        z[win["frame_index"]] = win["poses"]
    a = sc.pose_rms(np.r_[x0[:n0], z.reshape(-1)], ds, zt)
    b = sc.pose_rms(xt, ds, zt)
    print("static object: rms lagged %.3e, track %.3e, ratio %.3f" % (a, b, a / b))
    assert a < b, (a, b)


# ---- 12. the C++ driver ----
def test_find_solution_live_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    tool = str(tmp_path / "live_mapper_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "live_mapper_main.cpp"), "-o", tool, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    ds = aar.solution_read(os.path.join(folder, "initial.solution"))
    os.replace(os.path.join(folder, "initial.solution"), os.path.join(folder, "initial_tracking_only.solution"))
    lag = 3
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    run = subprocess.run(base + ["-live", str(lag), repr(SROT), repr(STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "live: " in run.stdout, run.stdout + run.stderr
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    n0, F = sc.ns(ds), ds.num_frames
    z = np.zeros((F, 6))
    with aar.Tracker(ds, lag=lag, smooth=True, sigma_rot=SROT, sigma_trans=STRANS, max_obs_per_frame=int(np.bincount(ds.obs_frame).max())) as t:
        for f in range(F):
            g = t.push(float(ds.frame_ids[f]), *frame_obs(ds, f), pose_init=ds.x_full[n0 + 6 * f: n0 + 6 * f + 6])
            if g["has_lagged"]:
                z[g["lagged_index"]] = g["lagged_pose"]
        win = t.window()
        z[win["frame_index"]] = win["poses"]
    # the file stores every pose as a 4x4 matrix and reads it back as the rotation vector of an angle below pi, while an LM step may carry a
    # frame's vector past pi: the same pose under another vector.  So the poses are compared as transforms, entry by entry
    zf = got.x_full[n0:].reshape(-1, 6)
    assert np.abs(tr.rodrigues(zf[:, :3]) - tr.rodrigues(z[:, :3])).max() < 1e-8 and np.abs(zf[:, 3:] - z[:, 3:]).max() < 1e-8
    assert np.abs(got.x_full[:n0] - ds.x_full[:n0]).max() < 1e-12
    assert np.abs(z - ds.x_full[n0:].reshape(-1, 6)).max() > 1e-6            # the frames have moved
    # the LiveTracker class itself: the same pushes by camera / marker ID, every frame started from the data set's pose
    out = subprocess.run([tool, os.path.join(folder, "initial_tracking_only.solution"), str(lag), repr(SROT), repr(STRANS)], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    kv = dict(l.split(" = ") for l in out.stdout.splitlines() if " = " in l)
    zc = np.array([[float(v) for v in kv["z%d" % f].split()] for f in range(F)])
    assert int(kv["frames"]) == F and np.abs(zc - z).max() < 1e-8
    # refused with the usage message: without -tracking-only, a lag out of range, one sigma only
    for bad in ([exe, folder, "0.05", "x", "-from-initial", "-live", "3", "0.05", "0.02"], base + ["-live", "16", "0.05", "0.02"],
                base + ["-live", "3", "0.05"], base + ["-live", "3", "0.05", "-1"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "live: " not in run.stdout, run.stdout
