"""The tracker bank (aar_tracker_bank_*: B live trackers in lockstep, member b = workgroup b of k_live_push_bank / k_live_init_bank, DESIGN.md
section 22) against the float64 restatements, against aar.Tracker member by member, and its contract.  Needs a real MI355X.

Bars, the project's own.  Against the restated push (tests/test_gpu_live_marginal.py's compare_push, imported): equal iteration, rejected-try and
stop codes, cost rtol 1e-10, poses 1e-9 + 2 slack, every restated margin above 1e-9.  Against aar_track at smooth = 0: 1e-12.  Uncertainty
(compare_marginal and the covariance test of the same file): marginal information 1e-8 of its largest entry, mean within the pose bar, covariance
blocks 1e-7 of the largest entry, sigma2 rtol 1e-10.  Start records (tests/test_gpu_live_detections.py): equal counts and sources, vote cost rtol
1e-11 / atol 1e-14, E_f at the two starts rtol 1e-10, start pose START_BAR.  The members and their measured margins: tests/live_bank_cases.py.

Member 2 of the raw-detection bank is fed frames of one detection and of 65 detections pooled from all frames of its scene: they disagree on the
object pose, so only its start record and its agreement with a single aar.Tracker are checked, not a restated refinement.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import aar
import live_bank_cases as bc
import live_marginal_restated as lm
import live_restated as lr
import smooth_cases as sc
import test_gpu_live_marginal as tm
import track_restated as tr
from test_gpu_live_detections import START_BAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def bank(members, lag, smooth, **over):
    return aar.TrackerBank([m.sol for m in members], **bc.bank_kw(members, lag, smooth, **over))


def push(k, members, f, time=None):
    return k.push(bc.TIMES[f] if time is None else time, bc.frames_of(members, f), bc.inits_of(members, f))


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


def run_member_bits(k, members, at, n, unc):
    """every push's result, window (and uncertainty record) of member `at` as bytes"""
    out = []
    for f in range(n):
        g = push(k, members, f)
        out.append((_rbits(g[at]), _wbits(k.window(at)), _ubits(k.uncertainty(at)) if unc else None))
    return out


# ---- 1. every member, every push, against the restated push ----
BANKS = {1: [1], 2: [2, 3], 5: [0, 1, 2, 3, 4]}


@pytest.mark.parametrize("lag,smooth", bc.MODES, ids=["lag%d-smooth%d" % m for m in bc.MODES])
@pytest.mark.parametrize("B", sorted(BANKS))
def test_every_member_every_push_against_the_restated_push(B, lag, smooth):
    members = [bc.member(i) for i in BANKS[B]]
    assert len({(m.ds.num_cams, m.ds.num_markers) for m in members}) == B              # heterogeneous
    n = bc.pushes(lag)
    with bank(members, lag, smooth) as k:
        assert len(k) == B
        for f in range(n):
            got = push(k, members, f)
            for b, m in enumerate(members):
                c = SimpleNamespace(name="B%d %s lag%d smooth%d" % (B, m.name, lag, smooth), lag=lag)
                tm.compare_push(c, f, got[b], bc.restated(m.index, lag, smooth)[f], k.window(b))
    if B == 5:
        slots = lag + 1
        for m in (members[1], members[4]):                                             # ring slots reused with fewer and (past lag 0's 4 pushes) more detections
            assert any(m.cnt[f] < m.cnt[f - slots] for f in range(slots, n)) and (lag == 0 or any(m.cnt[f] > m.cnt[f - slots] for f in range(slots, n)))
        assert 0 in members[2].cnt[1:n] and (lag == 0 or 1 in members[2].cnt[1:n])      # an empty and a one-detection frame inside the stream
        for f in range(1, n):                                                          # neighbours alternate pose_init and prediction, oppositely
            assert members[0].has_init[f] != members[1].has_init[f] and members[1].has_init[f] != members[2].has_init[f]


# ---- 2. isolation, bit for bit ----
@pytest.mark.parametrize("lag,tail", [(1, False), (3, True)], ids=["lag1-fixed", "lag3-marginal-cov"])
def test_a_member_gives_the_same_bytes_in_every_bank(lag, tail):
    target = bc.member(1)
    over = dict(anchor="marginal", covariance=True) if tail else {}
    n = bc.pushes(lag)

    def run(members, at):
        assert members[at] is target
        with bank(members, lag, True, **over) as k:
            return run_member_bits(k, members, at, n, tail)

    others = [bc.noisy(bc.member(0), 0), bc.noisy(target, 9), bc.noisy(bc.member(3), 3), bc.noisy(bc.member(4), 4)]       # (one shares the target's solution)
    alone = run([target], 0)
    for at in (0, 2, 4):
        members = others[:at] + [target] + others[at:4]
        assert len(members) == 5
        assert run(members, at) == alone, at
    crowd = [bc.tiny(j) for j in range(300)]
    crowd[150] = target
    assert run(crowd, 150) == alone                                                    # more workgroups than compute units
    # two banks fed the same pushes, and a bank after reset fed them again: every member's bytes
    members = [bc.member(i) for i in range(5)]
    with bank(members, lag, True, **over) as k1, bank(members, lag, True, **over) as k2:
        def every(k):
            out = []
            for f in range(n):
                g = push(k, members, f)
                out.append([(_rbits(g[b]), _wbits(k.window(b)), _ubits(k.uncertainty(b)) if tail else None) for b in range(5)])
            return out
        a, b2 = every(k1), every(k2)
        k1.reset()
        assert k1.window(3)["n"] == 0
        assert a == b2 and every(k1) == a


# ---- 3. against aar.Tracker, member by member ----
def test_smooth_0_is_track_member_by_member():
    members = [bc.member(i) for i in range(5)]
    want = []
    for m in members:
        with aar.Problem(m.ds) as p:
            xt, it, et = p.track(m.x0, aar.lm_default_params())
        want.append((xt[sc.ns(m.ds):].reshape(-1, 6), it, et))
    with bank(members, 0, False) as k:
        for f in range(bc.N):
            got = k.push(float(f), bc.frames_of(members, f), [m.td.z0[f] for m in members])
            for b, g in enumerate(got):
                zt, it, et = want[b]
                assert g["iterations"] == it[f] and g["window_frames"] == 1 and g["final_prior_cost"] == 0.0
                assert np.abs(g["pose"] - zt[f]).max() < 1e-12
                np.testing.assert_allclose(g["final_cost"], et[f], rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("lag,tail", [(1, False), (3, True)], ids=["lag1-fixed", "lag3-marginal-cov"])
def test_bank_against_single_trackers(lag, tail):
    members = [bc.member(i) for i in range(5)]
    over = dict(anchor="marginal", covariance=True) if tail else {}
    kw = bc.bank_kw(members, lag, True, **over)
    n = bc.pushes(lag)
    singles = [aar.Tracker(m.sol, **kw) for m in members]
    equal = True
    try:
        with aar.TrackerBank([m.sol for m in members], **kw) as k:
            for f in range(n):
                got = push(k, members, f)
                for b, m in enumerate(members):
                    s = singles[b].push(bc.TIMES[f], *m.frames[f], pose_init=m.td.z0[f] if m.has_init[f] else None)
                    g = got[b]
                    assert (g["iterations"], g["rejected_tries"], g["stop_code"], g["window_frames"]) == \
                        (s["iterations"], s["rejected_tries"], s["stop_code"], s["window_frames"])
                    np.testing.assert_allclose(g["final_cost"], s["final_cost"], rtol=1e-10, atol=1e-300)
                    assert np.abs(g["pose"] - s["pose"]).max() < 1e-9
                    ws, wb = singles[b].window(), k.window(b)
                    assert np.abs(wb["poses"] - ws["poses"]).max() < 1e-9
                    equal = equal and _rbits(g) == _rbits(s) and _wbits(wb) == _wbits(ws)
                    if tail:
                        us, ub = singles[b].uncertainty(), k.uncertainty(b)
                        for x in ("cov_valid", "window_frames", "has_marginal", "marginal_index", "marginal_dropped"):
                            assert us[x] == ub[x], x
                        np.testing.assert_allclose(ub["sigma2"], us["sigma2"], rtol=1e-10, atol=0.0)
                        if us["cov_valid"]:
                            assert np.abs(ub["cov"] - us["cov"]).max() <= 1e-7 * np.abs(us["cov"]).max()
                        if us["has_marginal"]:
                            assert np.abs(ub["marginal_info"] - us["marginal_info"]).max() <= 1e-8 * np.abs(us["marginal_info"]).max()
                            assert np.abs(ub["marginal_mean"] - us["marginal_mean"]).max() < 1e-9
                        equal = equal and _ubits(ub) == _ubits(us)
    finally:
        for t in singles:
            t.close()
    print("bank against single trackers, lag %d tail %d: every bit equal: %s" % (lag, tail, equal))


# ---- 4. marginalised anchor and covariance per member ----
@pytest.mark.parametrize("lag", [1, 3])
def test_uncertainty_per_member_against_the_restatement(lag):
    ids = [5, 1, 2]
    members = [bc.member(i) for i in ids]
    n = bc.pushes(lag)
    worst = 0.0
    with bank(members, lag, True, anchor="marginal", covariance=True) as k:
        for f in range(n):
            got = push(k, members, f)
            for b, m in enumerate(members):
                r = bc.restated(m.index, lag, True, "marginal")[f]
                win, u = k.window(b), k.uncertainty(b)
                tol = tm.compare_push(SimpleNamespace(name="%s marginal lag%d" % (m.name, lag), lag=lag), f, got[b], r, win)
                tm.compare_marginal(f, u, r, tol)
                assert list(u["frame_index"]) == list(win["frame_index"])
                cov, valid = lm.cov_blocks(r["problem"], win["poses"])
                assert u["cov_valid"] == int(valid) and u["cov"].shape == (win["n"], 6, 6)
                assert valid or (m.index == 5 and f == 0 and not u["cov"].any())       # only the push whose window is one empty frame has none
                if valid:
                    d = np.abs(u["cov"] - cov).max() / np.abs(cov).max()
                    worst = max(worst, d)
                    assert d <= 1e-7, (f, b, d)
                np.testing.assert_allclose(u["sigma2"], r["sigma2"], rtol=1e-10, atol=0.0)
        assert k.uncertainty(0)["marginal_dropped"] == 1 and k.uncertainty(1)["marginal_dropped"] == 0     # the stream that starts empty
    print("lag %d: largest covariance difference %.3e of the largest entry" % (lag, worst))


# ---- 5. raw detections ----
def _det_bank(policy, lag=1):
    mem = bc.det_members()
    k = aar.TrackerBank([c.sol for c, _, _ in mem], lag=lag, smooth=True, sigma_rot=bc.SROT, sigma_trans=bc.STRANS, max_obs_per_frame=70)
    k.enable_detections([dict(kw, start_policy=policy) for _, kw, _ in mem])
    return mem, k


def _det_single(c, kw, policy, lag=1):
    t = aar.Tracker(c.sol, lag=lag, smooth=True, sigma_rot=bc.SROT, sigma_trans=bc.STRANS, max_obs_per_frame=70)
    t.enable_detections(start_policy=policy, **kw)
    return t


@pytest.mark.parametrize("policy", ["vote", "best"])
def test_push_detections_per_member(policy):
    mem, k = _det_bank(policy)
    singles = [_det_single(c, kw, policy) for c, kw, _ in mem]
    lives = []
    for c, kw, frames in mem[:2]:
        cnt = [len(fr[0]) for fr in frames]
        ds = sc.copy_of(c.sol, num_frames=len(frames), obs_frame=np.repeat(np.arange(len(frames)), cnt).astype(np.int32),
                        obs_cam=np.concatenate([fr[0] for fr in frames]), obs_marker=np.concatenate([fr[1] for fr in frames]),
                        obs_uv=np.concatenate([fr[2] for fr in frames]))
        td = tr.TrackData(ds, np.r_[c.sol.x_full[:c.ns], np.zeros(6 * len(frames))])
        lives.append(lr.Live(td, lag=1, smooth=True, sigma_rot=bc.SROT, sigma_trans=bc.STRANS))
    seen, margin = set(), np.inf
    try:
        with k:
            for f in range(bc.DET_PUSHES):
                # under BEST member 0 also gets a pose_init on push 3: it competes as the prediction
                inits = [None] * 3
                if policy == "best" and f == 3:
                    inits[0] = singles[0].window()["poses"][-1] + 2e-3
                got, infos = k.push_detections(float(f), [fr[f] for _, _, fr in mem], inits)
                for b, (c, kw, frames) in enumerate(mem):
                    gs, si = singles[b].push_detections(float(f), *frames[f], pose_init=inits[b])
                    g, i = got[b], infos[b]
                    print("push %d member %d: candidates %d winner %d source %d cost %.12g" % (f, b, i["candidates"], i["winner"], i["start_source"], i["vote_cost"]))
                    for x in ("voted", "candidates", "winner", "start_source"):
                        assert i[x] == si[x], (f, b, x)
                    np.testing.assert_allclose(i["vote_cost"], si["vote_cost"], rtol=1e-11, atol=1e-14)
                    np.testing.assert_allclose([i["cost_prediction"], i["cost_vote"]], [si["cost_prediction"], si["cost_vote"]], rtol=1e-10, atol=0.0)
                    assert np.abs(i["start_pose"] - si["start_pose"]).max() <= START_BAR
                    assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (gs["iterations"], gs["rejected_tries"], gs["stop_code"])
                    assert np.abs(g["pose"] - gs["pose"]).max() < 1e-9
                    seen.add((b, i["candidates"]))
                    if b < 2:                                                          # the restatement runs along, from the start the device reports
                        r = lives[b].push(f, float(f), pose_init=i["start_pose"])
                        margin = min(margin, r["margin"])
                        assert r["margin"] > 1e-9
                        assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
                        np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-10)
                        assert np.abs(g["pose"] - r["pose"]).max() < 1e-9 + 2 * r["slack"]
    finally:
        for t in singles:
            t.close()
    assert (2, 1) in seen and (2, 65) in seen                                           # members with 1 and with 65 candidates
    print("policy %s: smallest restated margin %.2e" % (policy, margin))


def test_a_member_without_a_finite_candidate_rejects_the_first_push():
    mem, k = _det_bank("vote")
    frames = [fr[0] for _, _, fr in mem]
    bad = list(frames)
    nan = np.array(frames[1][2])
    nan[:, 0] = np.nan
    bad[1] = (frames[1][0], frames[1][1], nan)
    with k:
        before = k.stats()
        with pytest.raises(aar.AarError) as e:
            k.push_detections(0.0, bad)
        assert e.value.code == aar.AAR_ERR_NUMERIC and "member 1" in str(e.value), str(e.value)
        assert all(k.window(b)["n"] == 0 for b in range(3)) and k.stats()["pushes"] == before["pushes"]
        got, infos = k.push_detections(0.0, frames)
        w = [_wbits(k.window(b)) for b in range(3)]
    mem, fresh = _det_bank("vote")
    with fresh:
        want, winfos = fresh.push_detections(0.0, frames)
        assert [_rbits(g) for g in got] == [_rbits(g) for g in want]
        assert [i["start_pose"].tobytes() for i in infos] == [i["start_pose"].tobytes() for i in winfos]
        assert w == [_wbits(fresh.window(b)) for b in range(3)]


# ---- 6. rejected pushes ----
def test_rejected_pushes_leave_every_member_as_it_was():
    members = [bc.member(i) for i in range(5)]
    lag = 3
    cap = bc.bank_kw(members, lag, True)["max_obs_per_frame"]
    with bank(members, lag, True) as k, bank(members, lag, True) as clean:
        for f in range(6):
            push(k, members, f)
            push(clean, members, f)
        before = [_wbits(k.window(b)) for b in range(5)]
        pushes = k.stats()["pushes"]
        fr, init = bc.frames_of(members, 6), bc.inits_of(members, 6)

        def with_member(b, frame):
            return fr[:b] + [frame] + fr[b + 1:]

        cam, mk, uv = fr[2]
        big = (np.zeros(cap + 1, np.int32), np.zeros(cap + 1, np.int32), np.zeros((cap + 1, 8), np.float32))
        tries = [(("member 2", "obs_cam[%d]" % (len(cam) - 1)), lambda: k.push(bc.TIMES[6], with_member(2, (np.r_[cam[:-1], members[2].ds.num_cams], mk, uv)), init)),
                 (("member 4", "max_obs_per_frame"), lambda: k.push(bc.TIMES[6], with_member(4, big), init)),
                 (("frame_time",), lambda: k.push(bc.TIMES[5], fr, init)),
                 (("member 3", "pose_init[5]"), lambda: k.push(bc.TIMES[6], fr, init[:3] + [np.r_[members[3].td.z0[6][:5], np.nan]] + init[4:]))]
        for words, call in tries:
            with pytest.raises(aar.AarError) as e:
                call()
            assert e.value.code == aar.AAR_ERR_INVALID and all(w in str(e.value) for w in words), (words, str(e.value))
            assert [_wbits(k.window(b)) for b in range(5)] == before and k.stats()["pushes"] == pushes
        a, b = push(k, members, 6), push(clean, members, 6)
        assert [_rbits(g) for g in a] == [_rbits(g) for g in b]
    with bank(members, lag, True) as k:                                                 # the first push needs a start for every member
        with pytest.raises(aar.AarError) as e:
            k.push(0.0, bc.frames_of(members, 0), [members[0].td.z0[0], None] + [m.td.z0[0] for m in members[2:]])
        assert e.value.code == aar.AAR_ERR_INVALID and "member 1" in str(e.value) and "pose_init" in str(e.value)


# ---- 7. stats ----
def _delta(k, before):
    now = k.stats()
    return {x: now[x] - before[x] for x in now if x != "struct_size"}, now


def test_stats_count_copies_and_launches_per_push():
    members = [bc.member(i) for i in range(5)]
    with bank(members, 1, True) as k:
        st = k.stats()
        assert st["members"] == 5 and all(st[x] == 0 for x in st if x not in ("struct_size", "members")) and st["struct_size"] == 56
        assert k.stats(struct_size=24)["struct_size"] == 24
        for f in range(4):
            push(k, members, f)
            d, st = _delta(k, st)
            assert (d["pushes"], d["launches"], d["h2d_copies"], d["d2h_copies"]) == (1, 1, 1, 1)
            assert 0 < d["h2d_bytes"] <= 5 * (64 + 52 * k.prm.max_obs_per_frame + 15) and d["d2h_bytes"] == 5 * 40 * 8
    mem, k = _det_bank("vote")
    with k:
        st = k.stats()
        for f in range(3):
            k.push_detections(float(f), [fr[f] for _, _, fr in mem])
            d, st = _delta(k, st)
            # two launches; the first push without a pose_init reads the start records back before the refinement
            assert (d["pushes"], d["launches"], d["h2d_copies"], d["d2h_copies"]) == (1, 2, 1, 2 if f == 0 else 1)
        k.reset()
        k.enable_detections([dict(kw) for _, kw, _ in mem])
        z = [mem[b][0].ds.x_truth[mem[b][0].ns:][:6] for b in range(3)]
        k.push_detections(0.0, [fr[0] for _, _, fr in mem], z)                          # every member brings a pose_init: no read-back
        d, st = _delta(k, st)
        assert (d["pushes"], d["launches"], d["h2d_copies"], d["d2h_copies"]) == (1, 2, 1, 1)
