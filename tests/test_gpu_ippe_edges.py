"""d_ippe_square (csrc/ippe_vote.hpp) under k_ippe, k_live_init and k_live_init_bank on head-on and degenerate markers: the families of
tests/ippe_edge_cases.py against the independent float64 checker tests/ippe_reference.py, the truth and the oracle, at the bars
tests/test_ippe_reference_host.py holds the oracle to.  Needs a real MI355X.

Every family goes through aar.ippe_square in six launches: n = 1, 63, 64, 65 and 130 with the family's detections on the even places and
ordinary ones on the odd (a guard lane beside an ordinary one in a wavefront, a partial tail block), each over a fresh slice of the family, and
the remaining 337 in one launch -- 500 detections of the family in all.  One more launch per family has its corners distorted with DIST5, so
that d_undistort4 feeds the edge case.  Agreement with the oracle: atol 2e-6 on the matrices, rtol 1e-4 on the errors (tests/test_initializer.py).
"""
from types import SimpleNamespace

import numpy as np
import pytest

import aar
import ippe_edge_cases as ec
import ippe_reference as ir
import oracle_lib as O
from test_gpu_live_detections import _check_vote
from test_initializer import _compare_with_oracle, rigid, truth_transforms
from test_ippe_reference_host import assert_certified

pytestmark = pytest.mark.gpu

ZERO = np.zeros(5)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _against_oracle(label, g, o):
    dT = max(np.abs(g[0] - o[0]).max(), np.abs(g[2] - o[2]).max())
    with np.errstate(divide="ignore", invalid="ignore"):
        de = np.nanmax(np.r_[np.abs(g[1] / o[1] - 1), np.abs(g[3] / o[3] - 1), 0.0])      # (0 / 0: both exactly zero)
    print("%s: against the oracle: matrices %.3e, errors (relative) %.3e, bit-equal matrices %.4f" % (label, dT, de, np.mean(g[0] == o[0])))
    np.testing.assert_allclose(g[0], o[0], rtol=0, atol=2e-6)
    np.testing.assert_allclose(g[2], o[2], rtol=0, atol=2e-6)
    np.testing.assert_allclose(g[1], o[1], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(g[3], o[3], rtol=1e-4, atol=1e-9)


def _launch(label, uv, dist, truth, resid_bar, truth_bar):
    g = aar.ippe_square(ec.MS, ec.K, dist, uv)
    q = ir.normalise(ec.K, dist, uv)
    assert_certified(label, q, g[0], g[1], g[2], g[3], truth, resid_bar, truth_bar)
    _against_oracle(label, g, O.ippe_square(ec.MS, ec.K, dist, uv))


# ---- 1. aar.ippe_square on every family ----
@pytest.mark.parametrize("name", ec.FAMILIES)
def test_ippe_kernel_on_every_family_in_every_launch_shape(name):
    f, gen = ec.family(name), ec.family("generic")
    start = 0
    for n in ec.LAUNCH_SHAPES:
        uv, T, edge = ec.interleaved(f, n, start)
        start += int(edge.sum())
        g = aar.ippe_square(ec.MS, ec.K, ZERO, uv)
        q = ir.normalise(ec.K, ZERO, uv)
        # the family's bars on its places, the generic family's on the others
        for sel, rb, tb, who in ((edge, f.resid_bar, f.truth_bar, name), (~edge, gen.resid_bar, gen.truth_bar, "generic beside " + name)):
            if sel.any():
                assert_certified("%s n=%d" % (who, n), q[sel], g[0][sel], g[1][sel], g[2][sel], g[3][sel], T[sel], rb, tb)
        _against_oracle("%s n=%d" % (name, n), g, O.ippe_square(ec.MS, ec.K, ZERO, uv))
    assert start == 163
    _launch("%s rest" % name, f.uv[start:], ZERO, f.truth[start:], f.resid_bar, f.truth_bar)


@pytest.mark.parametrize("name", ec.FAMILIES)
def test_ippe_kernel_on_every_family_through_the_undistortion(name):
    f = ec.family(name)
    _launch("%s dist5" % name, ec.distorted(name), ec.DIST5, f.truth, f.resid_bar, f.truth_bar_dist)


def test_ippe_kernel_on_both_sides_of_the_pi_guard_seam():
    T, uv, guarded = ec.seam()
    _launch("seam", uv, ZERO, T, ec.RESID, ec.SEAM_TRUTH)


# ---- 2. the whole Initializer on the board scene (two cameras: the CamTab path of k_ippe) ----
def test_initializer_pipeline_on_the_board_scene():
    b = ec.board()
    out = aar.initializer_run(b.det, b.Ks, b.dists, b.ms, sizes=[ec.SIZE] * 2)
    r = O.init_run(b.det.num_cams, b.det.num_frames, b.det.det_frame, b.det.det_cam, b.det.det_id, b.det.det_uv, b.ms, b.Ks, b.dists)
    print("board: cameras %s markers %s frames %s, %d observations" % (list(out.cam_ids), list(out.marker_ids), list(out.frame_ids), out.num_obs))
    np.testing.assert_array_equal(out.cam_ids, [0, 1])
    np.testing.assert_array_equal(out.marker_ids, np.arange(6))
    np.testing.assert_array_equal(out.frame_ids, np.arange(5))
    assert out.num_obs == 60
    _compare_with_oracle(out, r, b.det, b.Ks, b.dists)
    sol = SimpleNamespace(num_cams=2, num_markers=6, num_frames=5, root_cam=0, root_marker=0, x_truth=out.x_full)
    cam, mk, fr = truth_transforms(sol)
    for k, got, truth in (("cameras", cam, b.T_cam), ("markers", mk, b.T_marker), ("frames", fr, b.T_object)):
        d = np.abs(np.array(got) - truth).max()
        print("%s: worst |T - truth| %.3e (bar %.1e)" % (k, d, b.truth_bar))
        assert d <= b.truth_bar


# ---- 3. the live path: camera 0 alone, every detection head-on ----
def _board_frames():
    b = ec.board()
    c = SimpleNamespace(ms=b.ms, K=b.Ks, dists=b.dists, cam=b.T_cam, mk=b.T_marker)
    frames = []
    for f in range(5):
        sel = (b.det.det_frame == f) & (b.det.det_cam == 0)
        assert sel.sum() == 6
        frames.append((b.det.det_cam[sel].copy(), b.det.det_id[sel].copy(), b.det.det_uv[sel].copy()))
    return b, c, frames


def test_live_tracker_and_bank_start_from_head_on_detections():
    b, c, frames = _board_frames()
    sol = ec.board_solution()
    bar = ec.BARS["fronto"]["truth_bar"]
    kw = dict(Ks=b.Ks, dists=b.dists, start_policy="vote")
    with aar.Tracker(sol, max_obs_per_frame=64) as t, aar.TrackerBank([sol], max_obs_per_frame=64) as bank:
        t.enable_detections(**kw)
        bank.enable_detections([kw])
        for f, (cam, mk, uv) in enumerate(frames):
            g, info = t.push_detections(float(f), cam, mk, uv)
            assert info["start_source"] == 2 and 6 <= info["candidates"] <= 12
            T, of = _check_vote(c, info, cam, mk, uv, 2.0)          # count, winner and cost against aar.ippe_square + aar.vote_transforms
            # (the start pose is the winner's 3x4 through rodrigues_mat2vec, whose half-turn branch keeps the axis of a float-rounded matrix to
            # about 1e-5 only -- 1.6e-5 on frame 4 -- so it is held to the truth, not to the winner's matrix)
            print("frame %d: start pose against the winner's matrix %.3e" % (f, np.abs(rigid(info["start_pose"]) - T[info["winner"]]).max()))
            d = np.abs(rigid(info["start_pose"]) - b.T_object[f]).max()
            dg = np.abs(rigid(g["pose"]) - b.T_object[f]).max()
            print("frame %d: start |T - truth| %.3e, refined %.3e (bar %.1e)" % (f, d, dg, bar))
            assert d <= bar and dg <= bar
            # one bank member on the same frame: k_live_init_bank
            gb, ib = bank.push_detections(float(f), [(cam, mk, uv)])
            for x in ("voted", "candidates", "winner", "start_source"):
                assert ib[0][x] == info[x], (f, x)
            np.testing.assert_allclose(ib[0]["vote_cost"], info["vote_cost"], rtol=1e-11, atol=1e-14)
            db = np.abs(rigid(ib[0]["start_pose"]) - b.T_object[f]).max()
            print("frame %d: bank start |T - truth| %.3e, against the tracker %.3e" % (f, db, np.abs(ib[0]["start_pose"] - info["start_pose"]).max()))
            assert db <= bar and np.abs(rigid(gb[0]["pose"]) - b.T_object[f]).max() <= bar
            np.testing.assert_allclose(rigid(ib[0]["start_pose"]), rigid(info["start_pose"]), rtol=0, atol=2e-6)
