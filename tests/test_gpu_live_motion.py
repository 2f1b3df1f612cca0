"""The live tracker's constant-velocity motion model (k_live_push_cv, the expected motions and the prediction formed on
the host) against the float64 restatement tests/live_motion_restated.py, and its contract.  Needs a real MI355X.

Bars: those of tests/test_gpu_live_tracker.py for the pushes (equal iteration, rejected-try and stop codes, final cost rtol 1e-10, poses
1e-9 + 2 slack, every restated margin above 1e-9) and of tests/test_gpu_live_marginal.py for the marginal (information 1e-8 of its largest
entry, the mean as a pose) and the covariance blocks (1e-7 of the largest entry, sigma2 rtol 1e-10).  The expected motion is formed in fp64 on
both sides from estimates that agree to the push's tolerance: rel against the restated rel 10 (1e-9 + 2 slack) (s <= 5 times the difference of
two estimates); velocity times the next time step against the next rel 1e-12 (host arithmetic alone); the cost at the start rtol 1e-9.  The coasting condition is the issue's: at every emptied frame the newest-pose
error with the model is at most a quarter of the random walk's, in rotation and in translation.

Measured on an MI355X while writing this test: see DESIGN.md section 25.
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import aar
import live_bank_cases as bc
import live_detection_cases as ld
import live_gate_cases as gc
import live_gate_restated as gr
import live_marginal_cases as mc
import live_marginal_restated as lm
import live_motion_cases as mcv
import live_motion_restated as mr
import smooth_cases as sc
import track_restated as tr
from conftest import PKG

pytestmark = pytest.mark.gpu

KINDS = ["counts", "huber", "far"]
CV = dict(model="cv")


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
def device(kind, lag, anchor, max_dt=0.0):
    """every push of a case on the device with the model and covariance on: [(result, uncertainty record, window, motion record, predict at
    the newest time, predict at the next push's time)]"""
    c = mc.case(kind, lag)
    out = []
    with tracker(c, anchor=anchor, covariance=True, motion=dict(model="cv", max_dt=max_dt)) as t:
        for f in range(c.n):
            g = push(t, c, f)
            nxt = t.predict(c.times[f + 1]) if f + 1 < c.n else None
            out.append((g, t.uncertainty(), t.window(), t.last_motion(), t.predict(c.times[f]), nxt))
    return out


def compare_push(c, f, g, r, win, cost_atol=1e-300):
    """tests/test_gpu_live_tracker.py's comparison of one push, plus the cost at the start"""
    print("%s push %d: W %d it %d/%d rej %d/%d exit %d/%d cost %.12g/%.12g start %.12g/%.12g margin %.2e slack %.2e" % (
        c.name, f, g["window_frames"], g["iterations"], r["iterations"], g["rejected_tries"], r["rejected"], g["stop_code"], r["exit"],
        g["final_cost"], r["err"], g["initial_cost"], r["initial"], r["margin"], r["slack"]))
    assert r["margin"] > 1e-9, (f, r["margin"])
    assert g["frame_index"] == f and g["window_frames"] == r["window_frames"]
    np.testing.assert_allclose(g["initial_cost"], r["initial"], rtol=1e-9, atol=cost_atol)
    assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
    np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-10, atol=cost_atol)
    np.testing.assert_allclose([g["final_data_cost"], g["final_prior_cost"]], [r["data"], r["prior"]], rtol=1e-9, atol=1e-12)
    tol = 1e-9 + 2 * r["slack"]
    assert np.abs(g["pose"] - r["pose"]).max() < tol
    assert (g["lagged_pose"] is None) == (r["lagged_pose"] is None)
    if r["lagged_pose"] is not None:
        assert g["lagged_index"] == f - c.lag and np.abs(g["lagged_pose"] - r["lagged_pose"]).max() < tol
    assert win["n"] == r["window_frames"] and np.abs(win["poses"] - r["window"]).max() < tol
    assert (win["anchor_pose"] is None) == (r["anchor"] is None)
    if r["anchor"] is not None:
        assert np.abs(win["anchor_pose"] - r["anchor"]).max() < tol
    Ef, Pe = r["problem"].costs(r["window"])
    np.testing.assert_allclose(win["frame_err"], Ef, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(win["pair_err"], Pe, rtol=1e-7, atol=1e-12)
    return tol


def compare_uncertainty(f, u, r, win, tol):
    """tests/test_gpu_live_marginal.py's comparisons of the marginal and of the covariance blocks"""
    assert u["has_marginal"] == r["has_marginal"] and u["marginal_index"] == r["marginal_index"] and u["marginal_dropped"] == r["dropped"]
    if r["has_marginal"]:
        Lr, mr_ = r["marginal"]
        dL = np.abs(u["marginal_info"] - Lr).max() / np.abs(Lr).max()
        dm = np.abs(u["marginal_mean"] - mr_).max()
        print("    marginal after push %d: info %.2e of its largest entry, mean %.2e" % (f, dL, dm))
        assert dL <= 1e-8 and dm < tol
    cov, valid = lm.cov_blocks(r["problem"], win["poses"])
    assert u["cov_valid"] == int(valid) and u["window_frames"] == win["n"]
    if valid:
        d = np.abs(u["cov"] - cov).max() / np.abs(cov).max()
        print("    covariance after push %d: %.2e of the largest entry" % (f, d))
        assert d <= 1e-7, (f, d)
    np.testing.assert_allclose(u["sigma2"], r["sigma2"], rtol=1e-10, atol=0.0)


def compare_motion(c, f, m, r, slack, max_dt=0.0):
    """slack: the largest of the restated stream: rel is s <= 5 times the difference of two estimates, each good to 1e-9 + 2 slack"""
    assert m["model"] == 1 and m["predicted"] == r["predicted"] and m["newest_time"] == c.times[f]
    assert np.abs(m["rel"] - r["rel"]).max() <= 10 * (1e-9 + 2 * slack)
    rule = f >= 2 and not (max_dt > 0 and (c.times[f] - c.times[f - 1] > max_dt or c.times[f - 1] - c.times[f - 2] > max_dt))
    assert m["predicted"] == int(rule) and bool(m["rel"].any()) == rule


# ---- 5. every push against the restated push ----
CASES = [(k, lag, a) for k in KINDS for lag in (0, 1, 3, 15) for a in ("fixed", "marginal") if not (a == "marginal" and lag == 0)]


@pytest.mark.parametrize("kind,lag,anchor", CASES, ids=["%s-lag%d-%s" % c for c in CASES])
def test_every_push_against_the_restated_push(kind, lag, anchor):
    c, ref, dev = mc.case(kind, lag), mcv.restated(kind, lag, anchor), device(kind, lag, anchor)
    from_prediction = 0
    slack = max(r["slack"] for r in ref)
    for f in range(c.n):
        g, u, win, m, _, _ = dev[f]
        r = ref[f]
        tol = compare_push(c, f, g, r, win)
        compare_uncertainty(f, u, r, win, tol)
        compare_motion(c, f, m, r, slack)
        if not c.has_init[f] and r["predicted"]:
            # the start is the prediction, not the previous estimate: the cost there is another one
            z_rw = r["start"].copy()
            z_rw[-1] = ref[f - 1]["pose"]
            if abs(r["problem"].cost(z_rw) - r["initial"]) > 1e-6 * r["initial"]:
                from_prediction += 1
    if not all(c.has_init):
        assert from_prediction > 0
    cnt = np.bincount(c.ds.obs_frame, minlength=c.n)
    if kind == "counts":
        assert 0 in cnt[1:-1] and 1 in cnt[1:-1]
    if kind == "far":
        assert sum(r["rejected"] for r in ref) > 0


# ---- 6. off is off ----
def _bits(g, win):
    return [g[k] for k in ("iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost", "final_prior_cost",
                           "final_mu")] + list(g["pose"]) + ([] if g["lagged_pose"] is None else list(g["lagged_pose"])) + \
        list(win["poses"].reshape(-1)) + list(win["frame_err"]) + list(win["pair_err"])


def _ubits(u):
    return [u[k] for k in ("cov_valid", "sigma2", "window_frames", "has_marginal", "marginal_index", "marginal_dropped")] + \
        list(u["frame_index"]) + list(u["cov"].reshape(-1)) + list(u["marginal_info"].reshape(-1)) + list(u["marginal_mean"])


def _stream_bits(c, t):
    out = []
    for f in range(c.n):
        g = push(t, c, f)
        out.append(_bits(g, t.window()) + _ubits(t.uncertainty()))
    return out


@pytest.mark.parametrize("anchor", ["fixed", "marginal"])
def test_random_walk_model_is_no_call_at_all(anchor):
    c = mc.case("counts", 3)
    with tracker(c, anchor=anchor, covariance=True) as t:
        plain = _stream_bits(c, t)
    with tracker(c, anchor=anchor, covariance=True, motion="rw") as t:
        assert _stream_bits(c, t) == plain
        for call in (t.last_motion, lambda: t.predict(c.times[-1] + 1.0)):  # the tracker has no model
            with pytest.raises(aar.AarError) as e:
                call()
            assert e.value.code == aar.AAR_ERR_INVALID and "no motion model" in str(e.value)
    with tracker(c, anchor=anchor, covariance=True, motion="cv") as t:      # ... and the model is not a no-op
        assert _stream_bits(c, t) != plain


# ---- 7. max_dt ----
@pytest.mark.parametrize("lag,anchor", [(0, "fixed"), (3, "marginal")])
def test_max_dt_between_the_short_and_the_long_gaps(lag, anchor):
    c, ref, dev = mc.case("counts", lag), mcv.restated("counts", lag, anchor, mcv.MAX_DT), device("counts", lag, anchor, mcv.MAX_DT)
    gaps = np.diff(c.times)
    assert gaps.min() < mcv.MAX_DT < gaps.max()
    for f in range(c.n):
        g, u, win, m, _, _ = dev[f]
        tol = compare_push(c, f, g, ref[f], win)
        compare_uncertainty(f, u, ref[f], win, tol)
        compare_motion(c, f, m, ref[f], max(r["slack"] for r in ref), mcv.MAX_DT)
    flags = [m["predicted"] for _, _, _, m, _, _ in dev]
    assert flags == [int(f >= 2 and gaps[f - 1] <= mcv.MAX_DT and gaps[f - 2] <= mcv.MAX_DT) for f in range(c.n)]
    assert 0 in flags[2:] and 1 in flags
    assert flags != [m["predicted"] for _, _, _, m, _, _ in device("counts", lag, anchor)]
    # past max_dt the prediction is the newest pose
    for f in range(c.n - 1):
        g, _, _, _, _, nxt = dev[f]
        if f >= 1:
            assert np.array_equal(nxt, g["pose"]) == bool(gaps[f] > mcv.MAX_DT)


# ---- 8. aar_tracker_last_motion and aar_tracker_predict ----
@pytest.mark.parametrize("lag", [0, 3])
def test_last_motion_and_predict(lag):
    c, ref, dev = mc.case("counts", lag), mcv.restated("counts", lag, "fixed"), device("counts", lag, "fixed")
    assert not dev[0][3]["velocity"].any() and not dev[0][3]["rel"].any() and np.array_equal(dev[0][5], dev[0][0]["pose"])
    checked = 0
    for f in range(c.n):
        g, _, win, m, now, nxt = dev[f]
        assert np.array_equal(now, g["pose"])                               # predict(t_n) is the newest pose
        if f >= 1:
            np.testing.assert_allclose(m["velocity"], ref[f]["velocity"], rtol=0, atol=2 * (1e-9 + 2 * max(ref[f]["slack"], ref[f - 1]["slack"])))
        if f + 1 < c.n:
            gn, _, _, mn, _, _ = dev[f + 1]
            if f >= 1:
                assert np.abs(m["velocity"] * (c.times[f + 1] - c.times[f]) - mn["rel"]).max() <= 1e-12
                want = mr.predict(g["pose"], m["velocity"], c.times[f], c.times[f + 1])
                assert np.abs(nxt - want).max() <= 1e-12                    # host math against numpy
            if not c.has_init[f + 1]:
                # the next push started from this prediction: the cost at its start is the restated cost there
                z0 = ref[f + 1]["start"].copy()
                z0[-1] = nxt
                np.testing.assert_allclose(gn["initial_cost"], ref[f + 1]["problem"].cost(z0), rtol=1e-9)
                checked += 1
    assert checked >= 5
    with tracker(c, motion="cv") as t:
        with pytest.raises(aar.AarError) as e:                              # before any push
            t.predict(0.0)
        assert e.value.code == aar.AAR_ERR_INVALID
        push(t, c, 0)
        push(t, c, 1)
        for bad in (c.times[1] - 0.5, float("nan")):                        # an earlier time, a time that is none
            with pytest.raises(aar.AarError) as e:
                t.predict(bad)
            assert e.value.code == aar.AAR_ERR_INVALID and "time" in str(e.value)


# ---- 9. raw detections and the gate ----
def _cv_stream(c, n=10, jump=4, noise=0.1, seed=4):
    """the detections of the scene's best-observed frame, projected along a constant-velocity trajectory that jumps once (a kidnap)"""
    f0 = int(np.argmax([len(f[0]) for f in c.frames]))
    cam, mk, _ = c.frames[f0]
    t = np.array([0.04 * f + 0.01 * (f % 3) for f in range(n)])             # uneven steps
    vel = np.r_[0.5 * np.array([0.6, -0.64, 0.48]), 0.25 * np.array([0.8, 0.0, -0.6])]     # per unit of time: about 0.02 rad and 10 mm per frame
    z = mcv.constant_velocity_poses(c.ds.x_truth[c.ns + 6 * f0:][:6], vel, t - t[n // 2])
    z[jump:] = mcv.constant_velocity_poses(z[jump] + np.array([0.25, -0.1, 0.15, 0.08, -0.05, 0.1]), vel, t[jump:] - t[jump])
    rng = np.random.default_rng(seed)
    return cam, mk, t, z, [ld.project(c, cam, mk, z[f], noise, rng) for f in range(n)]


@pytest.mark.parametrize("gated", [False, True])
def test_raw_detections_start_and_gate_at_the_prediction(gated):
    c = ld.case(False)
    cam, mk, times, zt, uvs = _cv_stream(c)
    seen = set()
    with aar.Tracker(c.sol, max_obs_per_frame=64, lag=3, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, motion="cv",
                     gate=gc.DEFAULT if gated else None) as t:
        t.enable_detections(Ks=c.K, dists=c.dists, start_policy="best")
        for f in range(len(times)):
            fd = ld.frame_data(c, cam, mk, uvs[f])
            pred = t.predict(times[f]) if f > 0 else None
            if f % 4 == 3:                                                  # a plain push in between: its start is the prediction as well
                g, info = t.push(times[f], cam, mk, uvs[f]), None
                start = pred
            else:
                g, info = t.push_detections(times[f], cam, mk, uvs[f])
                start = info["start_pose"]
                m = t.last_motion()
                if f == 0:
                    assert info["start_source"] == 2
                else:
                    Ep = tr.frame_error(fd, pred, -1.0)                     # START_BEST compares the vote with the motion prediction
                    print("frame %d: E prediction %.12g/%.12g vote %.12g source %d predicted %d" % (
                        f, info["cost_prediction"], Ep, info["cost_vote"], info["start_source"], m["predicted"]))
                    np.testing.assert_allclose(info["cost_prediction"], Ep, rtol=1e-10)
                    want = 2 if info["cost_vote"] < info["cost_prediction"] else (3 if m["predicted"] else 1)
                    assert info["start_source"] == want
                    if want != 2:
                        assert np.array_equal(start, pred)
                seen.add(info["start_source"])
            if gated:                                                       # the gate's e_d are taken at the start: the restated gate fed that z0
                want_e = gr.det_err(fd, start)
                want = gr.rule(want_e, **gc.DEFAULT)
                assert gc.margin(want_e, want), f
                e, keep = t.gate_detail()
                np.testing.assert_allclose(e, want_e, rtol=1e-10)
                assert np.array_equal(keep.astype(bool), want["keep"])
                gi = t.last_gate()
                assert (gi["gated"], gi["n_in"], gi["n_kept"]) == (want["gated"], want["n_in"], want["n_kept"])
            assert np.isfinite(g["pose"]).all()
    print("start sources seen:", sorted(seen))
    assert {2, 3} <= seen                                                   # the prediction wins on the trajectory, the vote at the jump


# ---- 10. the bank ----
def _mbits(m):
    return [m["model"], m["predicted"], m["newest_time"], m["rel"].tobytes(), m["velocity"].tobytes()]


def _gbits(g):
    return [g[x] for x in ("frame_index", "window_frames", "iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost",
                           "final_prior_cost", "final_mu", "has_lagged", "lagged_index")] + [g["pose"].tobytes(),
                                                                                             None if g["lagged_pose"] is None else g["lagged_pose"].tobytes()]


def _wbytes(w):
    return [w["n"], w["frame_index"].tobytes(), w["poses"].tobytes(), w["frame_err"].tobytes(), w["pair_err"].tobytes(),
            None if w["anchor_pose"] is None else w["anchor_pose"].tobytes()]


@pytest.mark.parametrize("lag,tail,gated", [(0, False, False), (1, False, True), (3, True, False)], ids=["lag0", "lag1-gated", "lag3-marginal-cov"])
def test_bank_member_is_a_single_tracker_with_the_model_bit_for_bit(lag, tail, gated):
    members = [bc.member(i) for i in (1, 2, 3)]                             # B = 3, unequal members (cameras, markers, detections per frame)
    assert len({(m.ds.num_cams, m.ds.num_markers, m.ds.num_obs) for m in members}) == 3
    over = dict(anchor="marginal", covariance=True) if tail else {}
    kw = bc.bank_kw(members, lag, True, **over)
    extra = dict(motion=dict(model="cv", max_dt=0.0), gate=gc.DEFAULT if gated else None)
    n = bc.pushes(lag)
    singles = [aar.Tracker(m.sol, **kw, **extra) for m in members]
    try:
        with aar.TrackerBank([m.sol for m in members], **kw, **extra) as k, aar.TrackerBank([m.sol for m in members], **kw, gate=extra["gate"]) as plain:
            with pytest.raises(aar.AarError) as e:
                k.enable_motion()                                           # a second call
            assert e.value.code == aar.AAR_ERR_INVALID and "already" in str(e.value)
            st, sp = k.stats(), plain.stats()
            differs = False
            for f in range(n):
                got = push_bank(k, members, f)
                ref = push_bank(plain, members, f)
                now, nowp = k.stats(), plain.stats()
                for x in ("pushes", "launches", "h2d_copies", "d2h_copies"):   # the launches and copies of the same bank without the model
                    assert now[x] - st[x] == nowp[x] - sp[x], (f, x)
                st, sp = now, nowp
                for b, m in enumerate(members):
                    s = singles[b].push(bc.TIMES[f], *m.frames[f], pose_init=m.td.z0[f] if m.has_init[f] else None)
                    assert _gbits(got[b]) == _gbits(s), (f, b)
                    assert _wbytes(k.window(b)) == _wbytes(singles[b].window()), (f, b)
                    assert _mbits(k.last_motion(b)) == _mbits(singles[b].last_motion()), (f, b)
                    assert np.array_equal(k.predict(b, bc.TIMES[f] + 0.5), singles[b].predict(bc.TIMES[f] + 0.5))
                    if tail:
                        assert _ubits(k.uncertainty(b)) == _ubits(singles[b].uncertainty()), (f, b)
                    if gated:
                        assert k.last_gate(b) == singles[b].last_gate()
                    differs = differs or _gbits(got[b]) != _gbits(ref[b])
            assert differs                                                  # the model is not a no-op in the bank
            assert any(k.last_motion(b)["predicted"] for b in range(3))
            # a rejected bank push leaves every member's motion state as it was
            before = [_mbits(k.last_motion(b)) for b in range(3)]
            fr, init = bc.frames_of(members, n - 1), bc.inits_of(members, n - 1)
            bad = max(range(3), key=lambda b: len(fr[b][0]))                    # a member with detections: one camera index out of range
            cam, mk, uv = fr[bad]
            cam = np.array(cam)
            cam[-1] = members[bad].ds.num_cams
            for call in (lambda: k.push(bc.TIMES[n - 1] + 1.0, fr[:bad] + [(cam, mk, uv)] + fr[bad + 1:], init),
                         lambda: k.push(bc.TIMES[n - 2], fr, init)):
                with pytest.raises(aar.AarError) as e:
                    call()
                assert e.value.code == aar.AAR_ERR_INVALID
                assert [_mbits(k.last_motion(b)) for b in range(3)] == before
            k.reset()                                                       # reset forgets the model
            with pytest.raises(aar.AarError) as e:
                k.last_motion(0)
            assert e.value.code == aar.AAR_ERR_INVALID and "no motion model" in str(e.value)
            if gated:
                k.enable_gate(**gc.DEFAULT)
            plain.reset()
            if gated:
                plain.enable_gate(**gc.DEFAULT)
            k.enable_motion(model="rw")                                     # ... and the random walk is no call at all
            for f in range(4):
                assert [_gbits(g) for g in push_bank(k, members, f)] == [_gbits(g) for g in push_bank(plain, members, f)]
    finally:
        for t in singles:
            t.close()


def push_bank(k, members, f):
    return k.push(bc.TIMES[f], bc.frames_of(members, f), bc.inits_of(members, f))


def test_bank_raw_detections_member_is_a_single_tracker_with_the_model():
    mem = bc.det_members()
    kw = dict(lag=1, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, max_obs_per_frame=70)
    singles = []
    try:
        with aar.TrackerBank([c.sol for c, _, _ in mem], motion="cv", **kw) as k:
            k.enable_detections([dict(d, start_policy="best") for _, d, _ in mem])
            for c, d, _ in mem:
                t = aar.Tracker(c.sol, motion="cv", **kw)
                t.enable_detections(start_policy="best", **d)
                singles.append(t)
            seen = set()
            for f in range(bc.DET_PUSHES):
                res, infos = k.push_detections(float(f), [fr[f] for _, _, fr in mem])
                for b, (c, d, fr) in enumerate(mem):
                    s, si = singles[b].push_detections(float(f), *fr[f])
                    assert _gbits(res[b]) == _gbits(s), (f, b)
                    assert infos[b]["start_source"] == si["start_source"] and np.array_equal(infos[b]["start_pose"], si["start_pose"]), (f, b)
                    assert _mbits(k.last_motion(b)) == _mbits(singles[b].last_motion())
                    seen.add(si["start_source"])
            print("start sources seen:", sorted(seen))
    finally:
        for t in singles:
            t.close()


# ---- 11. coasting on the device ----
def test_coasting_on_the_device():
    c = mcv.moving_stream()
    ref = mcv.coast_restated(True)
    runs = {}
    for model in ("cv", None):
        with tracker(c, motion=model) as t:
            runs[model] = []
            for f in range(c.n):
                g = t.push(c.times[f], *mc.frame_obs(c.ds, f), pose_init=c.truth[0] if f == 0 else None)
                runs[model].append((g, t.window()))
    # When all four window frames are empty (push 15) the cost is the prior's alone: pair errors e of about 1e-7 formed from rotations and
    # translations of order 1, so that fp64 leaves e a relative error of 1e-16 / 1e-7 and no two implementations agree on lam e^2 to rtol 1e-10.
    # The absolute floor is 2 lam e (eps |z|) per term = 2 * 2500 * 1e-7 * 7e-16, about 4e-19, times the window's 24 terms: 1e-17.
    for f in range(c.n):
        compare_push(c, f, runs["cv"][f][0], ref[f], runs["cv"][f][1], cost_atol=1e-17)
    for f in c.empty:
        (ar, at), (br, bt) = mcv.pose_errors(runs["cv"][f][0]["pose"], c.truth[f]), mcv.pose_errors(runs[None][f][0]["pose"], c.truth[f])
        print("frame %d: rotation %.3e / %.3e = %.4f, translation %.3e / %.3e = %.4f" % (f, ar, br, ar / br, at, bt, at / bt))
        assert ar <= 0.25 * br and at <= 0.25 * bt, f


# ---- 12. lifecycle ----
def test_enable_rules_reset_and_rejected_pushes():
    c = mc.case("counts", 3)
    want = [_bits(g, w) + _ubits(u) + list(m["rel"]) + list(m["velocity"]) + [m["predicted"]] for g, u, w, m, _, _ in device("counts", 3, "marginal")]
    cam, mk, uv = mc.frame_obs(c.ds, 2)
    with tracker(c, smooth=False, lag=0, sigma_rot=0.0, sigma_trans=0.0) as t:
        with pytest.raises(aar.AarError) as e:                              # no prior, nothing to carry the model
            t.enable_motion()
        assert e.value.code == aar.AAR_ERR_INVALID and "smooth" in str(e.value)
    with tracker(c, anchor="marginal", covariance=True) as t:
        for kw, field in ((dict(model=7), "model"), (dict(max_dt=-1.0), "max_dt"), (dict(max_dt=float("nan")), "max_dt")):
            with pytest.raises(aar.AarError) as e:
                t.enable_motion(**kw)
            assert e.value.code == aar.AAR_ERR_INVALID and field in str(e.value)
        short = aar.tracker_motion_params(struct_size=4)
        assert aar.lib().aar_tracker_enable_motion(t.handle, C.byref(short)) == aar.AAR_ERR_INVALID
        for rnd in range(2):
            t.enable_motion(max_dt=0.0)
            with pytest.raises(aar.AarError) as e:                          # a second call
                t.enable_motion()
            assert e.value.code == aar.AAR_ERR_INVALID and "already" in str(e.value)
            with pytest.raises(aar.AarError) as e:                          # before any push
                t.last_motion()
            assert e.value.code == aar.AAR_ERR_INVALID
            got = []
            for f in range(c.n):
                if f in (3, 9):                                             # rejected pushes leave the motion state as it was
                    before = t.last_motion()
                    for bad in (lambda: t.push(c.times[f], np.r_[cam[:-1], c.ds.num_cams], mk, uv, c.td.z0[f]),
                                lambda: t.push(c.times[f - 1], cam, mk, uv, c.td.z0[f])):
                        with pytest.raises(aar.AarError) as e:
                            bad()
                        assert e.value.code == aar.AAR_ERR_INVALID
                    after = t.last_motion()
                    assert all(np.array_equal(before[k], after[k]) for k in before)
                g = push(t, c, f)
                m = t.last_motion()
                got.append(_bits(g, t.window()) + _ubits(t.uncertainty()) + list(m["rel"]) + list(m["velocity"]) + [m["predicted"]])
            assert got == want, rnd                                         # the same pushes after a reset, the model enabled again: the same bits
            t.reset()
            with pytest.raises(aar.AarError) as e:                          # reset forgets the model
                t.last_motion()
            assert e.value.code == aar.AAR_ERR_INVALID and "no motion model" in str(e.value)
        plain = _stream_bits(c, t)                                          # after the reset, without the call: the random walk
    with tracker(c, anchor="marginal", covariance=True) as t:
        assert _stream_bits(c, t) == plain
    with tracker(c) as t:
        push(t, c, 0)
        with pytest.raises(aar.AarError) as e:                              # after a push
            t.enable_motion()
        assert e.value.code == aar.AAR_ERR_INVALID and "before the first push" in str(e.value)


# ---- the command line ----
def test_find_solution_motion_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    ds = aar.solution_read(os.path.join(folder, "initial.solution"))
    os.replace(os.path.join(folder, "initial.solution"), os.path.join(folder, "initial_tracking_only.solution"))
    lag, max_dt = 3, 1.5
    live = ["-live", str(lag), repr(mc.SROT), repr(mc.STRANS)]
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    for bad in (live + ["-motion"], live + ["-motion", "fast"], ["-live", "0", "-motion", "cv"], live + ["-motion", "cv", "nan"], ["-motion", "cv"]):
        run = subprocess.run(base + bad, capture_output=True, text=True, timeout=300)      # no model, an unknown one, no sigmas, no number, no -live
        assert run.returncode != 0 and "Usage" in run.stdout, (bad, run.stdout)
    run = subprocess.run(base + live + ["-motion", "cv", repr(max_dt), "-anchor", "marginal"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "live: " in run.stdout, run.stdout + run.stderr
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    n0, F = sc.ns(ds), ds.num_frames
    z, predicted = np.zeros((F, 6)), 0
    with aar.Tracker(ds, lag=lag, smooth=True, sigma_rot=mc.SROT, sigma_trans=mc.STRANS, anchor="marginal", motion=dict(model="cv", max_dt=max_dt),
                     max_obs_per_frame=int(np.bincount(ds.obs_frame).max())) as t:
        for f in range(F):
            t.push(float(ds.frame_ids[f]), *mc.frame_obs(ds, f), pose_init=ds.x_full[n0 + 6 * f: n0 + 6 * f + 6])
            predicted += t.last_motion()["predicted"]
            win = t.window()
            z[win["frame_index"]] = win["poses"]
    assert "motion: constant velocity, %d of %d pushes with an expected motion" % (predicted, F) in run.stdout, run.stdout
    zf = got.x_full[n0:].reshape(-1, 6)
    assert np.abs(tr.rodrigues(zf[:, :3]) - tr.rodrigues(z[:, :3])).max() < 1e-8 and np.abs(zf[:, 3:] - z[:, 3:]).max() < 1e-8
    rw = subprocess.run(base + live + ["-motion", "rw", "-anchor", "marginal"], capture_output=True, text=True, timeout=300)
    assert rw.returncode == 0 and "motion:" not in rw.stdout, rw.stdout + rw.stderr
    zr = aar.solution_read(os.path.join(folder, "final_tracking_only.solution")).x_full[n0:].reshape(-1, 6)
    assert np.abs(zr - zf).max() > 0                                        # the random walk gives other poses
