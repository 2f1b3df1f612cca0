"""The live tracker fed raw detections (aar_tracker_push_detections: k_live_init in front of k_live_push) against the
data-set path it replaces (aar_initializer_object_poses + aar_track), the oracle's Initializer, the existing IPPE / vote kernels and the float64
restatements tests/track_restated.py and tests/live_restated.py.  Needs a real MI355X.

Bars.  Start pose against aar_initializer_object_poses: START_BAR (the arithmetic up to the winner's 3x4 is the same code; only the 3x4 ->
(rvec, t) runs in device instead of host libm), and 2e-6 against the oracle, the bar tests/test_initializer.py holds.  Final pose of a push
against aar_track: FINAL_BAR, ten times the measured maximum (the issue's 1e-9 plus the start difference is looser).  Vote cost against aar_vote_transforms: rtol 1e-11, atol 1e-14 (test_vote_kernel_equals_oracle's bar; the atol carries the sets of one or two
candidates, whose costs are rounding noise around zero).
E_f at the two starts against track_restated.frame_error: rtol 1e-10.  Against live_restated: cost rtol 1e-10, poses 1e-9 + 2 slack.
"""
import numpy as np
import pytest

import aar
import live_detection_cases as ld
import live_restated as lr
import oracle_lib as O
import smooth_cases as sc
import track_restated as tr
from test_initializer import rigid

pytestmark = pytest.mark.gpu

START_BAR = 5.6e-15     # ten times the largest difference measured over test 1's two cases (5.551e-16, the dist8 case; nodist 4.441e-16)
FINAL_BAR = 4.5e-15     # ... and of the final poses against aar_track (4.441e-16, dist8; nodist 2.220e-16); iterations were equal
SROT, STRANS = 0.05, 0.02


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def tracker(c, policy="vote", threshold=None, min_detections=None, max_obs=64, **kw):
    t = aar.Tracker(c.sol, max_obs_per_frame=max_obs, **kw)
    t.enable_detections(Ks=c.K, dists=c.dists, ippe_threshold=threshold, min_detections=min_detections, start_policy=policy)
    return t


def data_set_path(c):
    """what the tracker replaces: the Initializer on the whole recording with the map fixed, then track() on every frame"""
    out = aar.initializer_run(c.det, c.K, c.dists, c.ms, solution=c.sol)
    with aar.Problem(out, optimize=(False, False, True)) as p:
        x, it, err = p.track(out.x_full)
    return out, x[c.ns:].reshape(-1, 6), it, err


def host_candidates(c, cam, mk, uv, threshold):
    """the candidate set of one frame rebuilt on the host from aar.ippe_square and the solution's transforms, in the reference's order:
    (T, T1inv, T2inv [n, 4, 4], the detection of every candidate)"""
    n = len(cam)
    T1 = np.zeros((n, 4, 4)); T2 = np.zeros((n, 4, 4)); e1 = np.zeros(n); e2 = np.zeros(n)
    for k in np.unique(cam):
        s = cam == k
        T1[s], e1[s], T2[s], e2[s] = aar.ippe_square(c.ms, c.K[k], c.dists[k], uv[s])
    with np.errstate(invalid="ignore", divide="ignore"):
        has2 = e2 / e1 < threshold
    order = sorted(range(n), key=lambda d: (mk[d], cam[d]))
    T, A, B, of = [], [], [], []
    for d in order:
        for P in ([T1[d], T2[d]] if has2[d] else [T1[d]]):
            with np.errstate(invalid="ignore"):
                T.append(c.cam[cam[d]] @ P @ O.inv4(c.mk[mk[d]])); A.append(c.mk[mk[d]] @ O.inv4(P)); B.append(O.inv4(c.cam[cam[d]]))
            of.append(d)
    return np.array(T), np.array(A), np.array(B), np.array(of)


# ---- 1. the reference's loop, frame by frame ----
@pytest.mark.parametrize("distorted", [False, True], ids=["nodist", "dist8"])
def test_every_frame_equals_initializer_then_track(distorted):
    c = ld.case(distorted)
    out, zt, it, err = data_set_path(c)
    _, _, zo = ld.oracle_object_poses(distorted)
    z0 = out.x_full[c.ns:].reshape(-1, 6)
    worst_start = worst_final = 0.0
    with tracker(c) as t:
        for f, (cam, mk, uv) in enumerate(c.frames):
            g, info = t.push_detections(float(f), cam, mk, uv)
            ds_, df_ = np.abs(info["start_pose"] - z0[f]).max(), np.abs(g["pose"] - zt[f]).max()
            worst_start, worst_final = max(worst_start, ds_), max(worst_final, df_)
            print("frame %d: candidates %d winner %d start diff %.3e (oracle %.3e) final diff %.3e it %d/%d" % (
                f, info["candidates"], info["winner"], ds_, np.abs(info["start_pose"] - zo[f]).max(), df_, g["iterations"], it[f]))
            assert info["voted"] == 1 and info["start_source"] == 2 and 0 <= info["winner"] < info["candidates"]
            assert len(cam) <= info["candidates"] <= 2 * len(cam)
            assert ds_ <= START_BAR
            assert np.abs(info["start_pose"] - zo[f]).max() < 2e-6
            assert df_ <= FINAL_BAR
            assert g["iterations"] == it[f] and g["window_frames"] == 1
            np.testing.assert_allclose(g["final_cost"], err[f], rtol=1e-9)
            assert info["cost_prediction"] == 0.0 and info["cost_vote"] == 0.0
    print("largest start difference %.3e, largest final difference %.3e" % (worst_start, worst_final))


# ---- 2. the vote's pieces against the existing kernels, at the loop edges ----
def _check_vote(c, info, cam, mk, uv, threshold):
    T, A, B, of = host_candidates(c, cam, mk, uv, threshold)
    best, weight, cost = aar.vote_transforms(c.ms, [0, len(T)], T, A, B)
    print("candidates %d/%d winner %d/%d cost %.15g/%.15g" % (info["candidates"], len(T), info["winner"], best[0], info["vote_cost"], weight[0]))
    assert info["voted"] == 1 and info["candidates"] == len(T) and info["winner"] == best[0]
    np.testing.assert_allclose(info["vote_cost"], weight[0], rtol=1e-11, atol=1e-14)
    return T, of


@pytest.mark.parametrize("threshold,counts", [(1e-30, (1, 63, 65, 129)), (1e30, (2, 64, 270))], ids=["first-only", "both"])
def test_vote_equals_the_existing_kernels_at_the_loop_edges(threshold, counts):
    c = ld.case(False)
    per = 1 if threshold < 1 else 2
    with tracker(c, threshold=threshold, min_detections=1, max_obs=140) as t:
        for k, want in enumerate(counts):
            cam, mk, uv = ld.pooled(c, want // per)
            g, info = t.push_detections(float(k), cam, mk, uv)       # (the first push waits for the vote, the others do not)
            assert info["candidates"] == want and info["start_source"] == 2
            T, of = _check_vote(c, info, cam, mk, uv, threshold)
            np.testing.assert_allclose(rigid(info["start_pose"]), T[info["winner"]], rtol=0, atol=2e-6)


def test_root_only_frame_and_a_frame_below_min_detections():
    c = ld.case(False)
    with tracker(c, min_detections=2) as t:
        cam, mk, uv = ld.root_only_detection(c, 2)                   # identity transforms on both sides
        g, info = t.push_detections(0.0, cam, mk, uv)
        T, of = _check_vote(c, info, cam, mk, uv, 2.0)
        P = aar.ippe_square(c.ms, c.K[cam[0]], c.dists[cam[0]], uv)
        assert any(np.array_equal(T[info["winner"]], X) for X in (P[0][0], P[0][1], P[2][0], P[2][1]))      # the candidate IS the IPPE pose
        # one detection, min_detections 2: no vote, the frame starts from the previous estimate / from pose_init
        g1, i1 = t.push_detections(1.0, cam[:1], mk[:1], uv[:1])
        assert (i1["voted"], i1["candidates"], i1["winner"], i1["start_source"]) == (0, 0, -1, 1) and np.array_equal(i1["start_pose"], g["pose"])
        zi = g["pose"] + 1e-3
        g2, i2 = t.push_detections(2.0, cam[:1], mk[:1], uv[:1], pose_init=zi)
        assert (i2["voted"], i2["start_source"]) == (0, 0) and np.array_equal(i2["start_pose"], zi)
    with tracker(c, min_detections=2) as t:                          # ... and on a first push nothing is left to start from
        with pytest.raises(aar.AarError) as e:
            t.push_detections(0.0, cam[:1], mk[:1], uv[:1])
        assert e.value.code == aar.AAR_ERR_INVALID and "min_detections" in str(e.value) and t.window()["n"] == 0


# ---- 3. NaN ----
def test_non_finite_detections_never_win_and_a_vote_without_a_winner_is_rejected():
    c = ld.case(False)
    cam, mk, uv = c.frames[2]
    bad = np.array(uv)
    bad[1, 3] = np.nan
    fin = np.arange(len(cam)) != 1
    with tracker(c, threshold=1e30) as t:
        # a first push on which no candidate is finite: rejected, the tracker stays empty and then takes a good push
        allbad = np.array(uv)
        allbad[:, 0] = np.nan
        with pytest.raises(aar.AarError) as e:
            t.push_detections(0.0, cam, mk, allbad)
        assert e.value.code == aar.AAR_ERR_NUMERIC and t.window()["n"] == 0
        g, info = t.push_detections(0.0, cam, mk, uv)
        assert g["frame_index"] == 0 and info["start_source"] == 2 and t.window()["n"] == 1
        # one non-finite corner: its candidate stays in the count but never wins; the others' sums stay finite and are those of the
        # finite candidates alone
        g, info = t.push_detections(1.0, cam, mk, bad)
        Tall, A, B, of = host_candidates(c, cam, mk, bad, 1e30)
        keep = of != 1
        best, weight, cost = aar.vote_transforms(c.ms, [0, int(keep.sum())], Tall[keep], A[keep], B[keep])
        assert info["candidates"] == len(of) == 2 * len(cam) - 1 and np.isfinite(info["vote_cost"])     # (its NaN error ratio keeps one solution)
        assert of[info["winner"]] != 1 and info["winner"] == np.nonzero(keep)[0][best[0]]
        np.testing.assert_allclose(info["vote_cost"], weight[0], rtol=1e-11, atol=1e-14)
        # a later vote without a winner falls back on the previous estimate
        win = t.window()
        g2, i2 = t.push_detections(2.0, cam, mk, allbad)
        assert (i2["voted"], i2["winner"], i2["start_source"]) == (1, -1, 1) and np.array_equal(i2["start_pose"], win["poses"][-1])


# ---- 4. policy BEST ----
def _undistorted(c, f):
    cam, mk, uv = c.frames[f]
    return cam, mk, uv                                             # (the undistorted case: raw corners are the data set's)


def test_best_policy_costs_and_choice():
    c = ld.case(False)
    out, zt, it, err = data_set_path(c)
    z0 = out.x_full[c.ns:].reshape(-1, 6)
    with tracker(c, policy="best", lag=3, smooth=True, sigma_rot=SROT, sigma_trans=STRANS) as t:
        prev = None
        seen = set()
        for f in range(8):
            cam, mk, uv = _undistorted(c, f)
            init = z0[f] + 2e-3 if f == 5 else None                 # a pose_init under BEST competes as the prediction
            g, info = t.push_detections(float(f), cam, mk, uv, pose_init=init)
            fd = ld.frame_data(c, cam, mk, uv)
            if f == 0:
                assert info["start_source"] == 2 and info["cost_prediction"] == 0.0 and info["cost_vote"] == 0.0
            else:
                pred = init if init is not None else prev
                Ep, Ev = tr.frame_error(fd, pred, -1.0), tr.frame_error(fd, z0[f], -1.0)
                print("frame %d: E pred %.12g/%.12g vote %.12g/%.12g source %d" % (f, info["cost_prediction"], Ep, info["cost_vote"], Ev, info["start_source"]))
                np.testing.assert_allclose(info["cost_prediction"], Ep, rtol=1e-10)
                np.testing.assert_allclose(info["cost_vote"], Ev, rtol=1e-10)
                want = 2 if info["cost_vote"] < info["cost_prediction"] else (0 if init is not None else 1)
                assert info["start_source"] == want
                assert np.array_equal(info["start_pose"], pred) if want != 2 else np.abs(info["start_pose"] - z0[f]).max() <= START_BAR
            seen.add(info["start_source"])
            prev = g["pose"]
    print("start sources seen:", sorted(seen))


def _kidnap(c, f):
    """a pose for frame f from another seed's trajectory, far from the track so far, whose detections the cameras can still see: the one
    that makes the restated cost at the prediction largest"""
    other = ld.case(False, seed=77)
    cam, mk, _ = c.frames[f]
    zprev = c.ds.x_truth[c.ns + 6 * (f - 1):][:6]
    best = None
    for k in range(other.ds.num_frames):
        z = other.ds.x_truth[other.ns + 6 * k:][:6]
        uv = ld.project(c, cam, mk, z)
        if not (np.all(np.isfinite(uv)) and np.all((uv > 0) & (uv < 1280))):
            continue
        E = tr.frame_error(ld.frame_data(c, cam, mk, uv), zprev, -1.0)
        if best is None or E > best[0]:
            best = (E, z)
    return best[1]


def test_best_policy_recovers_from_a_kidnap():
    c = ld.case(False)
    F, fk = 8, 5
    rng = np.random.default_rng(5)
    zk = _kidnap(c, fk)
    frames = [list(c.frames[f]) for f in range(F)]
    frames[fk][2] = ld.project(c, frames[fk][0], frames[fk][1], zk, noise=0.2, rng=rng)
    # the restatement runs along: every push from the start the device reports
    n = [len(fr[0]) for fr in frames]
    ds = sc.copy_of(c.sol, num_frames=F, obs_frame=np.repeat(np.arange(F), n).astype(np.int32), obs_cam=np.concatenate([fr[0] for fr in frames]),
                    obs_marker=np.concatenate([fr[1] for fr in frames]), obs_uv=np.concatenate([fr[2] for fr in frames]))
    td = tr.TrackData(ds, np.r_[c.sol.x_full[:c.ns], np.zeros(6 * F)])
    live = lr.Live(td, lag=3, smooth=True, sigma_rot=SROT, sigma_trans=STRANS)
    with tracker(c, policy="best", lag=3, smooth=True, sigma_rot=SROT, sigma_trans=STRANS) as t:
        prev = None
        for f in range(F):
            cam, mk, uv = frames[f]
            g, info = t.push_detections(float(f), cam, mk, uv)
            r = live.push(f, float(f), pose_init=info["start_pose"])
            print("frame %d: source %d E pred %.6g vote %.6g  it %d/%d cost %.12g/%.12g margin %.2e" % (
                f, info["start_source"], info["cost_prediction"], info["cost_vote"], g["iterations"], r["iterations"], g["final_cost"], r["err"], r["margin"]))
            assert r["margin"] > 1e-9
            assert (g["iterations"], g["rejected_tries"], g["stop_code"]) == (r["iterations"], r["rejected"], r["exit"])
            np.testing.assert_allclose(g["final_cost"], r["err"], rtol=1e-10)
            assert np.abs(g["pose"] - r["pose"]).max() < 1e-9 + 2 * r["slack"]
            if f == fk:
                fd = td.frame(f)
                Ep, Ev, Et = tr.frame_error(fd, prev, -1.0), tr.frame_error(fd, info["start_pose"], -1.0), tr.frame_error(fd, zk, -1.0)
                print("kidnap: restated E at the prediction %.6g, at the vote %.6g, at the truth %.6g" % (Ep, Ev, Et))
                assert Ep >= 10 * Ev and Ep >= 10 * Et              # the jump was chosen so that both margins hold
                assert info["start_source"] == 2
                assert np.abs(rigid(g["pose"]) - rigid(zk)).max() < 0.02
            prev = g["pose"]


# ---- 5. invariants ----
def _run(t, c, frames):
    return [t.push_detections(float(f), *c.frames[f]) for f in frames]


def _same(a, b):
    for (g1, i1), (g2, i2) in zip(a, b):
        for k in g1:
            if k != "seconds":
                assert np.array_equal(g1[k], g2[k]) if g1[k] is not None else g2[k] is None, k
        for k in i1:
            assert np.array_equal(i1[k], i2[k]), k


def test_same_pushes_same_bits_also_after_a_reset():
    c = ld.case(True)
    kw = dict(policy="best", lag=2, smooth=True, sigma_rot=SROT, sigma_trans=STRANS)
    with tracker(c, **kw) as t1, tracker(c, **kw) as t2:
        a, b = _run(t1, c, range(7)), _run(t2, c, range(7))
        _same(a, b)
        with pytest.raises(aar.AarError) as e:                       # enabling twice is refused
            t1.enable_detections(Ks=c.K, dists=c.dists)
        assert e.value.code == aar.AAR_ERR_INVALID
        t1.reset()
        assert t1.window()["n"] == 0
        with pytest.raises(aar.AarError):                            # the reset also forgets the enabling
            t1.push_detections(0.0, *c.frames[0])
        t1.enable_detections(Ks=c.K, dists=c.dists, start_policy="best")
        _same(a, _run(t1, c, range(7)))


def test_rejected_pushes_change_nothing():
    c = ld.case(False)
    cam, mk, uv = c.frames[0]
    with aar.Tracker(c.sol, max_obs_per_frame=max(len(f[0]) for f in c.frames[:3])) as t:
        with pytest.raises(aar.AarError) as e:                       # before enable_detections
            t.push_detections(0.0, cam, mk, uv)
        assert e.value.code == aar.AAR_ERR_INVALID and "enable_detections" in str(e.value) and t.window()["n"] == 0
        t.enable_detections(Ks=c.K, dists=c.dists)
        _run(t, c, range(2))
        before = t.window()
        for bad in ((np.r_[cam[:-1], c.ds.num_cams], mk, uv, "det_cam"), (cam, np.r_[mk[:-1], -1], uv, "det_marker"),
                    (np.r_[cam, cam, cam], np.r_[mk, mk, mk], np.r_[uv, uv, uv], "max_obs_per_frame")):
            with pytest.raises(aar.AarError) as e:
                t.push_detections(5.0, bad[0], bad[1], bad[2])
            assert e.value.code == aar.AAR_ERR_INVALID and bad[3] in str(e.value)
            after = t.window()
            for k in before:
                assert np.array_equal(before[k], after[k]), k
        g, info = t.push_detections(2.0, cam, mk, uv)
        assert g["frame_index"] == 2


def test_alternating_with_plain_pushes():
    c = ld.case(True)
    out, zt, it, err = data_set_path(c)                              # its obs_uv: the undistorted corners, frame by frame
    z0 = out.x_full[c.ns:].reshape(-1, 6)
    kw = dict(lag=2, smooth=True, sigma_rot=SROT, sigma_trans=STRANS)
    with tracker(c, **kw) as ta, aar.Tracker(c.sol, max_obs_per_frame=64, **kw) as tb:
        for f in range(8):
            cam, mk, raw = c.frames[f]
            und = out.obs_uv[np.asarray(out.obs_frame) == f]
            np.testing.assert_array_equal(out.obs_cam[np.asarray(out.obs_frame) == f], cam)
            if f % 2 == 0:
                ga, info = ta.push_detections(float(f), cam, mk, raw)
                start = info["start_pose"]
            else:
                start = z0[f]
                ga = ta.push(float(f), cam, mk, und, pose_init=start)
            gb = tb.push(float(f), cam, mk, und, pose_init=start)
            d = np.abs(ga["pose"] - gb["pose"]).max()
            print("frame %d: %s pose diff %.3e it %d/%d" % (f, "detections" if f % 2 == 0 else "plain", d, ga["iterations"], gb["iterations"]))
            assert d <= FINAL_BAR and ga["iterations"] == gb["iterations"]


# ---- 6. the driver ----
def test_find_solution_from_detections(tmp_path):
    import os
    import subprocess
    from conftest import PKG
    from test_host_logic import CALIB_YAML
    c = ld.case(False)
    exe = os.path.join(PKG, "aar_find_solution")
    folder = tmp_path / "run"
    folder.mkdir()
    aar.detections_write(str(folder / "aruco.detections"), c.ds)
    start = sc.copy_of(c.sol, x_full=np.r_[c.sol.x_full[:c.ns], np.zeros(6 * ld.FRAMES)])     # the map, and object poses that say nothing
    aar.solution_write(str(folder / "initial_tracking_only.solution"), start)
    for k in range(c.ds.num_cams):                                   # calib files: the scene's pinhole cameras, no distortion
        d = folder / ("cam_%d" % k)
        d.mkdir()
        K = c.K[k]
        (d / "calib.yml").write_text(
            "%YAML:1.0\n---\nimage_width: 1280\nimage_height: 720\ncamera_matrix: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [ "
            + ", ".join(repr(float(v)) for v in K.reshape(9)) + " ]\ndistortion_coefficients: !!opencv-matrix\n   rows: 1\n   cols: 5\n   dt: d\n"
            "   data: [ 0., 0., 0., 0., 0. ]\n")
    assert CALIB_YAML.startswith("%YAML")                            # (the dialect tests/test_host_logic.py reads)
    base = [exe, str(folder), repr(c.ms), "x", "-tracking-only", "-live", "0", "-from-detections"]
    run = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "live: %d pushes" % ld.FRAMES in run.stdout, run.stdout + run.stderr
    assert "votes: %d held, %d won" % (ld.FRAMES, ld.FRAMES) in run.stdout, run.stdout
    got = aar.solution_read(str(folder / "final_tracking_only.solution"))
    T = np.array([rigid(z) for z in got.x_full[c.ns:].reshape(-1, 6)])
    assert np.abs(T - c.fr).max() < 0.02
    assert np.abs(got.x_full[:c.ns] - c.sol.x_full[:c.ns]).max() < 1e-9
    run = subprocess.run(base + ["best"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "votes: %d held" % ld.FRAMES in run.stdout and "policy best" in run.stdout, run.stdout + run.stderr
    # other combinations are refused with the usage message
    for bad in ([exe, str(folder), repr(c.ms), "x", "-tracking-only", "-from-detections"], base + ["-from-initial"], base + ["-subseqs"]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "Usage:" in r.stdout
