"""The gate of the live trackers (aar_tracker_enable_gate: k_live_gate between a push's start and its refinement) against
the float64 restatement tests/live_gate_restated.py, against an ungated tracker fed the hand-filtered stream (bit for bit), and its contract.
Needs a real MI355X.

Bars, the project's own.  e_d, median, max and threshold against the restatement: rtol 1e-10, the bar tests/test_gpu_live_detections.py holds
for the same residuals summed into E_f; keep flags and every count exactly (tests/live_gate_cases.py's margin condition, asserted on the CPU in
tests/test_live_gate_host.py and here for the streams' device starts, makes them independent of rounding).  Against the restated LM
(live_gate_restated.GatedLive): equal iteration, rejected-try and stop codes, cost rtol 1e-10, poses 1e-9 + 2 slack, every restated margin above
1e-9 -- the bars of tests/test_gpu_live_detections.py for live_restated.  Raw and plain pushes of the same frame: FINAL_BAR of that file.
"""
import os
import subprocess

import numpy as np
import pytest

import aar
import live_detection_cases as ld
import live_gate_cases as gc
import live_gate_restated as gr
import smooth_cases as sc
from test_gpu_live_detections import FINAL_BAR
from test_initializer import rigid

pytestmark = pytest.mark.gpu

SROT, STRANS = 0.05, 0.02
MODES = [(0, False), (1, True), (3, True)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def kw_of(lag, smooth, **over):
    kw = dict(lag=lag, smooth=smooth, max_obs_per_frame=64)
    if smooth:
        kw.update(sigma_rot=SROT, sigma_trans=STRANS)
    kw.update(over)
    return kw


def _rbits(g):
    return [g[x] for x in ("frame_index", "window_frames", "iterations", "stop_code", "rejected_tries", "initial_cost", "final_cost", "final_data_cost",
                           "final_prior_cost", "final_mu", "has_lagged", "lagged_index")] + [g["pose"].tobytes(),
                                                                                             None if g["lagged_pose"] is None else g["lagged_pose"].tobytes()]


def _wbits(w):
    return [w["n"], w["frame_index"].tobytes(), w["poses"].tobytes(), w["frame_err"].tobytes(), w["pair_err"].tobytes(),
            None if w["anchor_pose"] is None else w["anchor_pose"].tobytes()]


def _ubits(u):
    return [u[x] for x in ("cov_valid", "sigma2", "window_frames", "has_marginal", "marginal_index", "marginal_dropped")] + \
        [u[x].tobytes() for x in ("frame_index", "cov", "marginal_info", "marginal_mean")]


def _gbits(g, e, k):
    return [g[x] for x in ("gated", "n_in", "n_kept", "n_nonfinite")] + [np.float64(g[x]).tobytes() for x in ("median", "max", "threshold")] + \
        [e.tobytes(), k.tobytes()]


def compare_gate(name, info, e, keep, want_e, want):
    """last_gate() / gate_detail() against the restated e_d and rule"""
    print("%s: n %d kept %d/%d nonfinite %d/%d median %.15g/%.15g max %.15g/%.15g threshold %.15g/%.15g" % (
        name, info["n_in"], info["n_kept"], want["n_kept"], info["n_nonfinite"], want["n_nonfinite"], info["median"], want["median"], info["max"],
        want["max"], info["threshold"], want["threshold"]))
    assert len(e) == len(keep) == len(want_e) == info["n_in"] == want["n_in"]
    fin = np.isfinite(want_e)
    assert np.array_equal(np.isfinite(e), fin)
    if fin.any():
        print("   largest relative e_d difference %.3e" % np.max(np.abs(e[fin] - want_e[fin]) / want_e[fin]))
    np.testing.assert_allclose(e[fin], want_e[fin], rtol=1e-10, atol=0)
    for k in ("median", "max", "threshold"):
        if np.isfinite(want[k]):
            np.testing.assert_allclose(info[k], want[k], rtol=1e-10, atol=0)
        else:
            assert info[k] == want[k], k
    assert np.array_equal(keep.astype(bool), want["keep"])
    assert (info["gated"], info["n_kept"], info["n_nonfinite"]) == (want["gated"], want["n_kept"], want["n_nonfinite"])


# ---- 1. the gate alone ----
@pytest.mark.parametrize("name", sorted(gc.frames()))
def test_gate_record_and_detail_against_the_restatement(name):
    c = gc.frames()[name]
    assert gc.margin(c.e, c.g)
    with aar.Tracker(gc.scene().sol, max_obs_per_frame=max(64, len(c.cam)), gate=c.rule) as t:
        g = t.push(0.0, c.cam, c.mk, c.uv, pose_init=c.z0)
        e, keep = t.gate_detail()
        compare_gate(name, t.last_gate(), e, keep, c.e, c.g)
        # the refinement saw the kept detections only: its data cost is the kept rows' at the final pose
        kept = gr.select(c.fd, c.g["keep"])
        np.testing.assert_allclose(g["final_data_cost"], gr.tr.frame_error(kept, g["pose"], -1.0), rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(t.window()["frame_err"][0], g["final_data_cost"], rtol=0, atol=0)


def test_gate_at_the_previous_estimate():
    c = gc.scene()
    st = gc.stream()
    with aar.Tracker(c.sol, gate=gc.DEFAULT, **kw_of(1, True)) as t:
        prev = t.push(gc.TIMES[0], *st[0][:3], pose_init=gc.perturbed(0))["pose"]
        for f in range(1, 6):
            cam, mk, uv, bad = st[f]
            fd = ld.frame_data(c, cam, mk, uv)
            want_e = gr.det_err(fd, prev)                     # the pose the device starts from, to the bit
            want = gr.rule(want_e, **gc.DEFAULT)
            assert gc.margin(want_e, want), f
            g = t.push(gc.TIMES[f], cam, mk, uv)
            e, keep = t.gate_detail()
            compare_gate("frame %d from the previous estimate" % f, t.last_gate(), e, keep, want_e, want)
            prev = g["pose"]


# ---- 2. bit for bit against a hand-filtered stream ----
def run_pair(kw, rule, frames, times, inits, unc):
    """a gated tracker on `frames` and an ungated one on the rows the gate kept (with the same pose_init): their bits must be equal"""
    c = gc.scene()
    seen = dict(rejected=0, want_rejected=0, emptied=0, small=0, slots=set())
    with aar.Tracker(c.sol, gate=rule, **kw) as tg, aar.Tracker(c.sol, **kw) as tu:
        for f, (cam, mk, uv) in enumerate(frames):
            gg = tg.push(times[f], cam, mk, uv, pose_init=inits[f])
            info = tg.last_gate()
            e, keep = tg.gate_detail()
            k = keep.astype(bool)
            if inits[f] is not None:                         # ... and the rows are those the restated rule keeps at that start
                want_e = gr.det_err(ld.frame_data(c, cam, mk, uv), inits[f])
                want = gr.rule(want_e, **rule)
                assert gc.margin(want_e, want) and np.array_equal(k, want["keep"]), f
                seen["want_rejected"] += want["n_in"] - want["n_kept"]
            assert info["n_kept"] == k.sum() and info["n_in"] == len(cam)
            gu = tu.push(times[f], cam[k], mk[k], uv[k], pose_init=inits[f])
            assert _rbits(gg) == _rbits(gu), f
            assert _wbits(tg.window()) == _wbits(tu.window()), f
            if unc:
                assert _ubits(tg.uncertainty()) == _ubits(tu.uncertainty()), f
            seen["rejected"] += int((~k).sum())
            seen["emptied"] += int(info["gated"] == 1 and k.sum() == 0 and len(cam) > 0)
            seen["small"] += int(info["gated"] == 0 and len(cam) > 0)
            seen["slots"].add(f % (kw["lag"] + 1))
    return seen


STREAM_RUNS = [(0, False, {}, "default"), (1, True, {}, "default"), (3, True, {}, "default"),
               (3, True, dict(anchor="marginal", covariance=True), "default"), (1, True, dict(with_huber=True, huber_delta=2.5), "default"),
               (1, True, {}, "emptying"), (0, False, {}, "emptying"), (2, True, dict(anchor="marginal", covariance=True), "emptying")]


@pytest.mark.parametrize("lag,smooth,over,rule", STREAM_RUNS,
                         ids=["lag%d-smooth%d-%s-%s" % (r[0], r[1], "-".join(sorted(r[2])) or "plain", r[3]) for r in STREAM_RUNS])
def test_gated_equals_hand_filtered_bit_for_bit(lag, smooth, over, rule):
    st = gc.stream()
    n = len(st)
    assert n >= 9 and n >= 2 * (lag + 1) + 1                 # every ring slot is reused
    frames = [s[:3] for s in st]
    inits = [gc.perturbed(f) for f in range(n)]
    seen = run_pair(kw_of(lag, smooth, **over), gc.DEFAULT if rule == "default" else gc.EMPTYING, frames, gc.TIMES, inits, bool(over.get("covariance")))
    print(seen)
    assert seen["small"] == 1 and seen["slots"] == set(range(lag + 1))
    if rule == "default":
        assert seen["rejected"] == seen["want_rejected"] >= 5 and seen["emptied"] == 0      # (at least the five misread ids, hundreds of px off)
    else:
        assert seen["emptied"] == n - 1


def test_compaction_across_chunks_bit_for_bit():
    fr = gc.frames()
    order = ["n300-pert", "n4096-odd", "n300-truth", "even-pert", "n300-pert"]      # a ring slot reused with more and with fewer records
    frames = [(fr[k].cam, fr[k].mk, fr[k].uv) for k in order]
    inits = [fr[k].z0 for k in order]
    for rule in (gc.DEFAULT, gc.FIXED):
        seen = run_pair(kw_of(0, False, max_obs_per_frame=4096), rule, frames, [float(i) for i in range(len(order))], inits, False)
        assert seen["rejected"] == seen["want_rejected"] > 2048
    for k in ("n300-pert", "n300-truth", "n4096-odd"):      # kept records cross the boundaries between the chunks of 256
        src = np.nonzero(fr[k].g["keep"])[0]
        dst = np.arange(len(src))
        assert np.any(src // 256 != dst // 256) and np.any((src // 256 == dst // 256) & (src != dst)), k


# ---- 3. against the restated LM ----
@pytest.mark.parametrize("lag,smooth", [(0, False), (3, True)], ids=["lag0", "lag3"])
def test_against_the_restated_gated_push(lag, smooth):
    c = gc.scene()
    st = gc.stream()
    live = gr.GatedLive(lag=lag, smooth=smooth, sigma_rot=SROT, sigma_trans=STRANS, **gc.DEFAULT)
    with aar.Tracker(c.sol, gate=gc.DEFAULT, **kw_of(lag, smooth)) as t:
        prev = None
        for f in range(9):
            cam, mk, uv, bad = st[f]
            fd = ld.frame_data(c, cam, mk, uv)
            init = gc.perturbed(0) if f == 0 else None       # after the first push every frame starts from the previous estimate
            g = t.push(gc.TIMES[f], cam, mk, uv, pose_init=init)
            r = live.push(fd, gc.TIMES[f], pose_init=init)
            e, keep = t.gate_detail()
            assert gc.margin(r["det_err"], r["gate"]), f
            want_e = gr.det_err(fd, init if f == 0 else prev)                        # e_d at the device's own start, to the bit
            compare_gate("frame %d" % f, t.last_gate(), e, keep, want_e, r["gate"] if f == 0 else dict(gr.rule(want_e, **gc.DEFAULT)))
            assert np.array_equal(keep.astype(bool), r["gate"]["keep"]), f
            print("frame %d: it %d/%d cost %.12g/%.12g margin %.2e slack %.2e pose diff %.3e" % (
                f, g["iterations"], r["iterations"], g["final_cost"], r["err"], r["margin"], r["slack"], np.abs(g["pose"] - r["pose"]).max()))
            assert r["margin"] > 1e-9
            assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
            np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-10)
            np.testing.assert_allclose(g["final_data_cost"], r["data"], rtol=1e-10)
            assert np.abs(g["pose"] - r["pose"]).max() < 1e-9 + 2 * r["slack"]
            w = t.window()
            zr, _ = live.live.window()
            assert np.abs(w["poses"] - zr).max() < 1e-9 + 2 * r["slack"]
            prev = g["pose"]


# ---- 4. raw detections ----
def undistorted(c, cam, uv):
    out = np.array(uv, dtype=np.float32)
    for k in np.unique(cam):
        out[cam == k] = aar.undistort_points(c.K[k], c.dists[k], uv[cam == k])
    return out


@pytest.mark.parametrize("distorted", [False, True], ids=["nodist", "dist8"])
@pytest.mark.parametrize("policy", ["vote", "best"])
def test_raw_detections_keep_exactly_the_planted_inliers(policy, distorted):
    c = ld.case(distorted)
    st = gc.stream(distorted)
    live = gr.GatedLive(lag=2, smooth=True, sigma_rot=SROT, sigma_trans=STRANS, **gc.DEFAULT)
    with aar.Tracker(c.sol, gate=gc.DEFAULT, **kw_of(2, True)) as t:
        t.enable_detections(Ks=c.K, dists=c.dists, start_policy=policy)
        for f in range(8):
            cam, mk, raw, bad = st[f]
            g, si = t.push_detections(gc.TIMES[f], cam, mk, raw)
            info = t.last_gate()
            e, keep = t.gate_detail()
            print("frame %d: source %d kept %d/%d median %.4g max %.4g threshold %.4g" % (
                f, si["start_source"], info["n_kept"], info["n_in"], info["median"], info["max"], info["threshold"]))
            if info["gated"]:
                assert np.array_equal(keep.astype(bool), ~bad), f
            else:
                assert len(cam) < gc.DEFAULT["min_detections"] and keep.all()
            fd = ld.frame_data(c, cam, mk, undistorted(c, cam, raw))
            r = live.push(fd, gc.TIMES[f], pose_init=si["start_pose"])
            assert gc.margin(r["det_err"], r["gate"]) and np.array_equal(keep.astype(bool), r["gate"]["keep"]), f
            fin = np.isfinite(r["det_err"])
            np.testing.assert_allclose(e[fin], r["det_err"][fin], rtol=1e-10)
            assert r["margin"] > 1e-9
            assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
            np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-10)
            assert np.abs(g["pose"] - r["pose"]).max() < 1e-9 + 2 * r["slack"]


def test_a_gated_raw_push_is_three_launches():
    c = gc.scene()
    st = gc.stream()
    with aar.TrackerBank([c.sol], gate=gc.DEFAULT, **kw_of(1, True)) as k:
        k.enable_detections()
        for f in range(3):
            before = k.stats()
            k.push_detections(gc.TIMES[f], [st[f][:3]])
            after = k.stats()
            assert after["launches"] - before["launches"] == 3 and after["h2d_copies"] - before["h2d_copies"] == 1
            assert after["d2h_copies"] - before["d2h_copies"] == (2 if f == 0 else 1)      # (the first raw push without pose_init reads its start)
            assert k.last_gate(0)["n_kept"] == int((~st[f][3]).sum())


# ---- 5. gate off ----
def test_an_ungated_tracker_is_untouched():
    c = gc.scene()
    st = gc.stream()
    kw = kw_of(2, True, anchor="marginal", covariance=True)

    def ungated():
        out = []
        with aar.Tracker(c.sol, **kw) as t:
            for f in range(8):
                g = t.push(gc.TIMES[f], *st[f][:3], pose_init=gc.perturbed(f) if f % 2 == 0 else None)
                out.append((_rbits(g), _wbits(t.window()), _ubits(t.uncertainty())))
            with pytest.raises(aar.AarError) as e:
                t.last_gate()
            assert e.value.code == aar.AAR_ERR_INVALID
            with pytest.raises(aar.AarError) as e:
                t.gate_detail()
            assert e.value.code == aar.AAR_ERR_INVALID
        return out

    a = ungated()
    with aar.Tracker(c.sol, gate=gc.DEFAULT, **kw) as t:
        for f in range(4):
            t.push(gc.TIMES[f], *st[f][:3], pose_init=gc.perturbed(f))
    assert ungated() == a
    # an ungated bank launches what it launched before: 1 per plain push, 2 per raw push, and copies the same bytes back
    with aar.TrackerBank([c.sol, c.sol], **kw_of(1, True)) as k:
        k.enable_detections()
        k.push(gc.TIMES[0], [st[0][:3]] * 2, [gc.perturbed(0)] * 2)
        s1 = k.stats()
        k.push_detections(gc.TIMES[1], [st[1][:3]] * 2)
        s2 = k.stats()
        assert s1["launches"] == 1 and s2["launches"] == 3 and s2["d2h_copies"] == 2 and s2["d2h_bytes"] == 2 * 2 * 40 * 8
        with pytest.raises(aar.AarError) as e:
            k.last_gate(0)
        assert e.value.code == aar.AAR_ERR_INVALID


# ---- 6. the bank ----
BANK_PLANS = [[(1, "id")], [(0, "rot"), (3, "shift"), (5, "id"), (6, "shift")], [], None, [(2, "shift")]]     # None: the object is not seen


def bank_frames(f):
    """member b's frame f: the clean frame with its own outliers; member 3 sees nothing, member 4 three detections (below min_detections)"""
    cam, mk, uv = gc.scene().frames[f]
    out = []
    for b, plan in enumerate(BANK_PLANS):
        if plan is None:
            out.append((cam[:0], mk[:0], uv[:0]))
        elif b == 4:
            out.append(gc.plant(cam[:3], mk[:3], uv[:3], plan)[:3])
        else:
            out.append(gc.plant(cam, mk, uv, [(i + (f % 2), kind) for i, kind in plan])[:3])
    return out


def bank_init(f):
    return gc.perturbed(f) if f == 0 or f % 3 == 2 else None


def test_every_bank_member_equals_a_single_gated_tracker():
    c = gc.scene()
    n, B = 8, len(BANK_PLANS)
    kw = kw_of(2, True, anchor="marginal", covariance=True)
    single = []
    for b in range(B):
        out = []
        with aar.Tracker(c.sol, gate=gc.DEFAULT, **kw) as t:
            for f in range(n):
                g = t.push(gc.TIMES[f], *bank_frames(f)[b], pose_init=bank_init(f))
                out.append((_rbits(g), _wbits(t.window()), _ubits(t.uncertainty()), _gbits(t.last_gate(), *t.gate_detail())))
        single.append(out)
    rejected = [sum(o[3][1] - o[3][2] for o in out) for out in single]
    print("rejected by member:", rejected)
    assert len(set(rejected)) >= 3 and rejected[2] == 0 and rejected[3] == 0 and rejected[4] == 0 and rejected[1] > rejected[0] > 0

    def run(members):
        out = []
        with aar.TrackerBank([c.sol] * len(members), gate=gc.DEFAULT, **kw) as k:
            for f in range(n):
                before = k.stats()
                fr = bank_frames(f)
                g = k.push(gc.TIMES[f], [fr[b] for b in members], [bank_init(f)] * len(members))
                after = k.stats()
                assert after["launches"] - before["launches"] == 2                       # the ungated push's one launch plus the gate
                assert after["h2d_copies"] - before["h2d_copies"] == 1 and after["d2h_copies"] - before["d2h_copies"] == 1
                out.append([(_rbits(g[i]), _wbits(k.window(i)), _ubits(k.uncertainty(i)), _gbits(k.last_gate(i), *k.gate_detail(i)))
                            for i in range(len(members))])
        return out

    five = run(list(range(B)))
    for b in range(B):
        assert [o[b] for o in five] == single[b], b
        assert [o[0] for o in run([b])] == single[b], b


# ---- 7. state ----
def test_reset_rejected_pushes_and_ordering():
    c = gc.scene()
    st = gc.stream()
    kw = kw_of(2, True)

    def run(t):
        out = []
        for f in range(6):
            g = t.push(gc.TIMES[f], *st[f][:3], pose_init=gc.perturbed(f) if f % 2 == 0 else None)
            out.append((_rbits(g), _wbits(t.window()), _gbits(t.last_gate(), *t.gate_detail())))
        return out

    with aar.Tracker(c.sol, **kw) as t:
        with pytest.raises(aar.AarError) as e:               # before any push
            t.enable_gate(**gc.DEFAULT)
            t.last_gate()
        assert e.value.code == aar.AAR_ERR_INVALID and "no push" in str(e.value)
        with pytest.raises(aar.AarError) as e:               # twice
            t.enable_gate(**gc.DEFAULT)
        assert e.value.code == aar.AAR_ERR_INVALID and "already" in str(e.value)
        a = run(t)
        # a rejected push leaves the window, the counts and the gate record as they were
        before = (_wbits(t.window()), _gbits(t.last_gate(), *t.gate_detail()))
        cam, mk, uv = st[6][:3]
        for bad, word in (((np.r_[cam[:-1], c.ds.num_cams], mk, uv), "obs_cam"), ((cam, np.r_[mk[:-1], -1], uv), "obs_marker"),
                          ((np.tile(cam, 7), np.tile(mk, 7), np.tile(uv, (7, 1))), "max_obs_per_frame")):
            with pytest.raises(aar.AarError) as e:
                t.push(gc.TIMES[6], *bad)
            assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value)
            assert (_wbits(t.window()), _gbits(t.last_gate(), *t.gate_detail())) == before
        with pytest.raises(aar.AarError) as e:
            t.push(gc.TIMES[2], cam, mk, uv)                 # the time does not ascend
        assert e.value.code == aar.AAR_ERR_INVALID and (_wbits(t.window()), _gbits(t.last_gate(), *t.gate_detail())) == before
        g6 = t.push(gc.TIMES[6], cam, mk, uv)                # ... and the stream goes on: the window holds the compacted frames
        assert g6["frame_index"] == 6
        t.reset()
        with pytest.raises(aar.AarError) as e:               # the reset forgets the gate
            t.last_gate()
        assert e.value.code == aar.AAR_ERR_INVALID
        t.enable_gate(**gc.DEFAULT)
        assert run(t) == a
    with aar.Tracker(c.sol, **kw) as t:                      # after a push
        t.push(gc.TIMES[0], *st[0][:3], pose_init=gc.perturbed(0))
        with pytest.raises(aar.AarError) as e:
            t.enable_gate(**gc.DEFAULT)
        assert e.value.code == aar.AAR_ERR_INVALID and "before the first push" in str(e.value)
    with aar.Tracker(c.sol, max_obs_per_frame=5000) as t:
        with pytest.raises(aar.AarError) as e:
            t.enable_gate(**gc.DEFAULT)
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED and "5000" in str(e.value)
    with aar.TrackerBank([c.sol], max_obs_per_frame=5000) as k:
        with pytest.raises(aar.AarError) as e:
            k.enable_gate(**gc.DEFAULT)
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    with aar.TrackerBank([c.sol, c.sol], **kw) as k:
        k.enable_gate(**gc.DEFAULT)
        with pytest.raises(aar.AarError) as e:
            k.enable_gate(**gc.DEFAULT)
        assert e.value.code == aar.AAR_ERR_INVALID
        with pytest.raises(aar.AarError) as e:
            k.last_gate(0)
        assert e.value.code == aar.AAR_ERR_INVALID
        k.push(gc.TIMES[0], [st[0][:3]] * 2, [gc.perturbed(0)] * 2)
        with pytest.raises(aar.AarError) as e:
            k.last_gate(2)
        assert e.value.code == aar.AAR_ERR_INVALID and "member" in str(e.value)
        with pytest.raises(aar.AarError) as e:               # a rejected bank push: all or nothing, the records stay
            k.push(gc.TIMES[1], [st[1][:3], (st[1][0], st[1][1] + 100, st[1][2])], [None, None])
        assert e.value.code == aar.AAR_ERR_INVALID and k.last_gate(1)["n_in"] == len(st[0][0]) and k.window(1)["n"] == 1


def test_gated_plain_and_raw_pushes_mixed():
    c = gc.scene()
    st = gc.stream()
    kw = kw_of(2, True)
    with aar.Tracker(c.sol, gate=gc.DEFAULT, **kw) as ta, aar.Tracker(c.sol, gate=gc.DEFAULT, **kw) as tb:
        ta.enable_detections(Ks=c.K, dists=c.dists)
        for f in range(8):
            cam, mk, uv, bad = st[f]                         # (no lens distortion in this scene: the raw corners are the undistorted ones)
            if f % 2 == 0:
                ga, si = ta.push_detections(gc.TIMES[f], cam, mk, uv)
                start = si["start_pose"]
            else:
                start = gc.truth(f)
                ga = ta.push(gc.TIMES[f], cam, mk, uv, pose_init=start)
            gb = tb.push(gc.TIMES[f], cam, mk, uv, pose_init=start)
            ia, ib = ta.last_gate(), tb.last_gate()
            d = np.abs(ga["pose"] - gb["pose"]).max()
            print("frame %d: %s kept %d/%d pose diff %.3e it %d/%d" % (f, "raw" if f % 2 == 0 else "plain", ia["n_kept"], ib["n_kept"], d,
                                                                      ga["iterations"], gb["iterations"]))
            assert np.array_equal(ta.gate_detail()[1], tb.gate_detail()[1]) and ia["n_kept"] == ib["n_kept"]
            if ia["gated"]:
                assert np.array_equal(ta.gate_detail()[1].astype(bool), ~bad)
            assert d <= FINAL_BAR and ga["iterations"] == gb["iterations"]


# ---- 8. the driver ----
def test_find_solution_live_gate(tmp_path):
    from conftest import PKG
    c = gc.scene()
    st = gc.stream()
    exe = os.path.join(PKG, "aar_find_solution")
    folder = tmp_path / "run"
    folder.mkdir()
    n = [len(s[0]) for s in st]
    rec = sc.copy_of(c.ds, obs_frame=np.repeat(np.arange(ld.FRAMES), n).astype(np.int32), obs_cam=np.concatenate([s[0] for s in st]),
                     obs_marker=np.concatenate([s[1] for s in st]), obs_uv=np.concatenate([s[2] for s in st]))
    aar.detections_write(str(folder / "aruco.detections"), rec)
    start = sc.copy_of(c.sol, x_full=np.r_[c.sol.x_full[:c.ns], np.zeros(6 * ld.FRAMES)])     # the map, and object poses that say nothing
    aar.solution_write(str(folder / "initial_tracking_only.solution"), start)
    for k in range(c.ds.num_cams):                                   # calib files: the scene's pinhole cameras, no distortion
        d = folder / ("cam_%d" % k)
        d.mkdir()
        (d / "calib.yml").write_text(
            "%YAML:1.0\n---\nimage_width: 1280\nimage_height: 720\ncamera_matrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [ "
            + ", ".join(repr(float(v)) for v in c.K[k].reshape(9)) + " ]\ndistortion_coefficients: !!opencv-matrix\n   rows: 1\n   cols: 5\n   dt: d\n"
            "   data: [ 0., 0., 0., 0., 0. ]\n")
    base = [exe, str(folder), repr(c.ms), "x", "-tracking-only", "-live", "3", repr(SROT), repr(STRANS), "-from-detections"]
    run = subprocess.run(base + ["-gate", "6", "3"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "live: %d pushes" % ld.FRAMES in run.stdout, run.stdout + run.stderr
    planted = sum(int(s[3].sum()) for f, s in enumerate(st) if f not in gc.SHORT)
    frames = sum(1 for f, s in enumerate(st) if s[3].any() and f not in gc.SHORT)
    assert "gate: %d detections rejected in %d frames" % (planted, frames) in run.stdout, run.stdout
    got = aar.solution_read(str(folder / "final_tracking_only.solution"))
    T = np.array([rigid(z) for z in got.x_full[c.ns:].reshape(-1, 6)])
    err = np.abs(T - c.fr).reshape(ld.FRAMES, -1).max(axis=1)
    print("largest transform entry off the truth, by frame:", " ".join("%.2e" % v for v in err))
    # against the truth, at the bar test_find_solution_from_detections holds for clean data: the frames that left the window (lag 3) before the
    # short frame arrived.  That frame is below min_detections and keeps its 40 px outlier among three detections by the rule, so it and the
    # frames the prior ties to it are held to the Python run below, not to the truth.
    short = min(gc.SHORT)
    assert short - 4 >= 1 and err[:short - 3].max() < 0.02
    assert np.abs(got.x_full[:c.ns] - c.sol.x_full[:c.ns]).max() < 1e-9
    # ... and its poses are those of the same pushes through the Python binding: every frame ends at its lagged estimate
    with aar.Tracker(c.sol, gate=dict(k_median=6, min_px=3), **kw_of(3, True)) as t:
        t.enable_detections(Ks=c.K, dists=c.dists)
        z = np.zeros((ld.FRAMES, 6))
        for f in range(ld.FRAMES):
            g, _ = t.push_detections(float(c.ds.frame_ids[f]), *st[f][:3])
            if g["lagged_pose"] is not None:
                z[g["lagged_index"]] = g["lagged_pose"]
        w = t.window()
        z[w["frame_index"]] = w["poses"]
    Tz = np.array([rigid(v) for v in z])
    print("driver against the Python run: poses %.3e, transforms %.3e" % (np.abs(got.x_full[c.ns:].reshape(-1, 6) - z).max(), np.abs(T - Tz).max()))
    assert np.abs(T - Tz).max() < 0.02                               # (compared as that test compares: transforms, 0.02)
    assert np.abs(got.x_full[c.ns:].reshape(-1, 6) - z).max() < 1e-9   # the same library fed the same pushes; the file keeps the doubles
    # -gate needs -live, and two numbers
    for bad in ([exe, str(folder), repr(c.ms), "x", "-tracking-only", "-gate", "6", "3"], base + ["-gate", "6"], base + ["-gate", "0", "0"]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0, r.stdout
