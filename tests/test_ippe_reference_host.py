"""The oracle's square-marker IPPE (oracle/init_oracle.cpp) on head-on and degenerate markers, against the independent float64 checker
tests/ippe_reference.py, on the families of tests/ippe_edge_cases.py (CPU only; tests/test_gpu_ippe_edges.py holds the kernels to the same bars).

Three guards separate the restatement (and csrc/ippe_vote.hpp) from aruco's ippe.cpp, which is wrong on these inputs: Rv = I when the centre
maps exactly onto the principal point, the radicands of the rotations' third row clamped at 0, and within 1e-3 rad of pi the rotation stored as
it stands instead of through IPPERot2vec + cv::Rodrigues.  Without them the oracle gives non-finite poses or stores a matrix (often the
identity) other than the one whose error it reports, on hundreds of the detections below.

Bars: ippe_edge_cases.BARS (the residuals of the two defining equations, |T1 - truth|), ippe_reference.ORTHO_BAR, ippe_reference.ERR_BAR.
"""
import functools

import numpy as np
import pytest

import ippe_edge_cases as ec
import ippe_reference as ir
import oracle_lib as O

ZERO = np.zeros(5)


@functools.lru_cache(maxsize=None)
def oracle_on(name, dist5=False):
    f = ec.family(name)
    uv = ec.distorted(name) if dist5 else f.uv
    dist = ec.DIST5 if dist5 else ZERO
    return uv, ir.normalise(ec.K, dist, uv), O.ippe_square(ec.MS, ec.K, dist, uv)


def assert_certified(label, q, T1, e1, T2, e2, truth, resid_bar, truth_bar):
    """everything the issue asks of a batch of IPPE results: finite, the checker, e1 <= e2, the truth; no case skipped"""
    n = len(q)
    assert T1.shape == T2.shape == (n, 4, 4) and e1.shape == e2.shape == (n,)
    nonfinite = int(np.sum(~(np.isfinite(T1).all(axis=(1, 2)) & np.isfinite(T2).all(axis=(1, 2)) & np.isfinite(e1) & np.isfinite(e2))))
    bad = ir.failures(ec.MS, q, T1, e1, resid_bar) + ir.failures(ec.MS, q, T2, e2, resid_bar)
    d = np.abs(T1 - truth).max(axis=(1, 2))
    r1, r2 = ir.check(ec.MS, q, T1), ir.check(ec.MS, q, T2)
    with np.errstate(invalid="ignore"):
        print("%s: n %d non-finite %d failures %d; worst rot %.3e trans %.3e ortho %.3e |e - e64| %.3e; |T1 - truth| %.3e (bar %.1e)" % (
            label, n, nonfinite, len(bad), np.nanmax(np.r_[r1.rot, r2.rot]), np.nanmax(np.r_[r1.trans, r2.trans]),
            np.nanmax(np.r_[r1.ortho, r2.ortho]), np.nanmax(np.r_[np.abs(e1 - r1.e64), np.abs(e2 - r2.e64)]), np.nanmax(d), truth_bar))
    assert nonfinite == 0
    assert not bad, bad[:10]
    assert np.all(e1 <= e2)
    assert np.all(d <= truth_bar), (int(np.argmax(d)), float(d.max()))
    for T in (T1, T2):                                    # float-rounded, as getRTMatrix's CV_32F conversion leaves them
        np.testing.assert_array_equal(T, T.astype(np.float32).astype(np.float64))


# ---- 1. the oracle on every family ----
@pytest.mark.parametrize("dist5", [False, True], ids=["nodist", "dist5"])
@pytest.mark.parametrize("name", ec.FAMILIES)
def test_oracle_passes_the_checker_on_every_family(name, dist5):
    f = ec.family(name)
    uv, q, (T1, e1, T2, e2) = oracle_on(name, dist5)
    assert len(uv) == ec.N
    assert_certified(name, q, T1, e1, T2, e2, f.truth, f.resid_bar, f.truth_bar_dist if dist5 else f.truth_bar)


def test_the_families_are_what_they_say():
    """the edge cases are edge cases: angles at pi, exact zeros of the centre, integer pixels"""
    ang = lambda T: np.arccos(np.clip((np.trace(T[:, :3, :3], axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert np.all(np.pi - ang(ec.family("fronto").truth) < 1e-7) and np.all(np.pi - ang(ec.family("integer").truth) < 1e-7)
    d = np.pi - ang(ec.family("near_pi").truth)
    assert d.max() < 1.1e-2 and np.sum(d < 1e-6) > 100 and np.sum(d > ec.DELTA0) > 50
    on = ec.family("on_axis")
    q = ir.normalise(ec.K, ZERO, on.uv[:ec.N // 2])
    assert np.array_equal(q[:, 0], -q[:, 2]) and np.array_equal(q[:, 1], -q[:, 3])       # p = q = 0 exactly: the 0 / 0 of ippe.cpp
    one = ec.family("one_axis")
    q = ir.normalise(ec.K, ZERO, one.uv[:ec.N // 2])
    c = q.sum(axis=1)
    assert np.all((c[:, 0] == 0) != (c[:, 1] == 0))
    for name, lo, hi in (("generic", 0, 60), ("oblique", 60, 85), ("grazing", 85, 89)):
        T = ec.family(name).truth
        ray = T[:, :3, 3] / np.linalg.norm(T[:, :3, 3], axis=1, keepdims=True)
        tilt = np.rad2deg(np.arccos(-(T[:, :3, 2] * ray).sum(axis=1)))
        assert lo - 1e-6 <= tilt.min() and tilt.max() <= hi + 1e-6, (name, tilt.min(), tilt.max())
    def side(f):            # the longer diagonal / sqrt 2: the side in pixels, whatever the tilt does to the other diagonal
        uv = f.uv.astype(np.float64)
        return np.maximum(np.linalg.norm(uv[:, 0:2] - uv[:, 4:6], axis=1), np.linalg.norm(uv[:, 2:4] - uv[:, 6:8], axis=1)) / np.sqrt(2)
    assert side(ec.family("small")).max() < 6.5 and side(ec.family("large")).min() > 150 and side(ec.family("far")).max() < 3
    assert np.all(ec.family("far").truth[:, 2, 3] == 20.0)


# ---- 2. the seam of the pi guard ----
def test_both_sides_of_the_pi_guard_seam():
    """true angles pi - 0.9, 0.999, 1.001 and 1.1 times delta0: the direct store and the round trip both satisfy the defining equations at float
    rounding and report the error of the matrix they store.  (Agreement with the TRUTH is limited by the conditioning of a head-on pose in
    float corners, 2.2e-5 on both sides: SEAM_TRUTH; what pins the stored matrix to float rounding is the checker.)"""
    T, uv, guarded = ec.seam()
    assert guarded.sum() == (~guarded).sum() == len(T) // 2
    ca = (np.trace(T[:, :3, :3], axis1=1, axis2=2) - 1) / 2
    assert np.all((ca <= -1 + ec.DELTA0 ** 2 / 2) == guarded)
    q = ir.normalise(ec.K, ZERO, uv)
    T1, e1, T2, e2 = O.ippe_square(ec.MS, ec.K, ZERO, uv)
    assert_certified("seam", q, T1, e1, T2, e2, T, ec.RESID, ec.SEAM_TRUTH)
    r = ir.check(ec.MS, q, T1)
    for side in (guarded, ~guarded):
        # a head-on J is a scaled rotation (condition 1): the residual is the float rounding of R, 6e-8 an entry, a few entries deep
        assert r.rot[side].max() < 1e-6 and r.trans[side].max() < 1e-6


# ---- 3. the board scene through the whole Initializer ----
def test_oracle_initializer_recovers_the_board_scene():
    b = ec.board()
    assert len(b.det.det_frame) == 60
    r = O.init_run(b.det.num_cams, b.det.num_frames, b.det.det_frame, b.det.det_cam, b.det.det_id, b.det.det_uv, b.ms, b.Ks, b.dists)
    np.testing.assert_array_equal(r["cam_ids"], [0, 1])
    np.testing.assert_array_equal(r["marker_ids"], np.arange(6))
    np.testing.assert_array_equal(r["frame_ids"], np.arange(5))
    np.testing.assert_array_equal(r["kept_frame_ids"], np.arange(5))
    for k, truth in (("T_cam", b.T_cam), ("T_marker", b.T_marker), ("T_object", b.T_object)):
        d = np.abs(r[k] - truth).max()
        print("%s: worst |T - truth| %.3e (bar %.1e)" % (k, d, b.truth_bar))
        assert d <= b.truth_bar
    # and its detections one by one: camera 0's are head-on
    q = ir.normalise(ec.K, ZERO, b.det.det_uv)
    T1, e1, T2, e2 = O.ippe_square(b.ms, ec.K, ZERO, b.det.det_uv)
    assert_certified("board detections", q, T1, e1, T2, e2, b.T_det, ec.RESID, ec.BARS["fronto"]["truth_bar"])


# ---- 4. planted faults: the checker sees each of them ----
def _round_trip(R):
    """IPPERot2vec + cv::Rodrigues without the guard, in numpy"""
    w = np.arccos((R[0, 0] + R[1, 1] + R[2, 2] - 1.0) / 2.0)
    rv = 1 / (2 * np.sin(w)) * w * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    th = np.linalg.norm(rv)
    if not th >= np.finfo(float).eps:
        return np.eye(3)
    a = rv / th
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(a, a) + np.sin(th) * S


def _stored(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32).astype(np.float64)


def _every_case_fails(q, T, e, resid_bar=ec.RESID):
    hit = set(i for i, _, _ in ir.failures(ec.MS, q, T, e, resid_bar))
    return len(hit), len(q)


def test_planted_unguarded_round_trip_fails_at_1e_minus_7():
    rng = np.random.default_rng(5)
    T, uv = [], []
    for i in range(40):
        ax = rng.uniform(0, 2 * np.pi)
        T.append(ec.rigid(ec.axis_angle([np.cos(ax), np.sin(ax), 0], np.pi - 1e-7), ec._centre(rng, rng.uniform(0.3, 3.0), 100)))
        uv.append(ec.corners(T[-1]).reshape(8))
    T, uv = np.array(T), np.array(uv, dtype=np.float32)
    q = ir.normalise(ec.K, ZERO, uv)
    T1, e1, T2, e2 = O.ippe_square(ec.MS, ec.K, ZERO, uv)
    assert _every_case_fails(q, T1, e1)[0] == 0                     # the guarded store passes ...
    # ... and the pose the parent stored does not: the same rotation (here the truth's, to which T1 agrees) through the round trip
    Tb = np.array([_stored(_round_trip(T[i, :3, :3]), T1[i, :3, 3]) for i in range(len(T))])
    assert np.abs(Tb - T1).max() > 1e-3
    assert _every_case_fails(q, Tb, e1) == (40, 40)


def test_planted_identity_for_a_half_turn_fails():
    f = ec.family("fronto")
    uv, q, (T1, e1, T2, e2) = oracle_on("fronto")
    Tb = T1.copy()
    Tb[:, :3, :3] = np.eye(3)
    assert _every_case_fails(q, Tb, e1) == (ec.N, ec.N)


def test_planted_rotation_by_1e_minus_4_fails():
    # on the oblique family, where a turn of the rotation shows at first order in equation (1) (head-on it does not: the ambiguity of IPPE)
    uv, q, (T1, e1, T2, e2) = oracle_on("oblique")
    rng = np.random.default_rng(9)
    Tb = T1.copy()
    for i in range(len(Tb)):
        Tb[i, :3, :3] = (ec.axis_angle(Tb[i, :3, 3], 1e-4 * (1 if i % 2 else -1)) @ Tb[i, :3, :3]).astype(np.float32)     # about the viewing ray
    assert _every_case_fails(q, Tb, e1) == (ec.N, ec.N)
    Tc = T1.copy()
    for i in range(len(Tc)):
        Tc[i, :3, :3] = (ec.axis_angle(rng.standard_normal(3), 1e-4) @ Tc[i, :3, :3]).astype(np.float32)                  # about any axis
    hit, n = _every_case_fails(q, Tc, e1)
    print("a random turn of 1e-4 rad: %d of %d fail" % (hit, n))
    assert hit >= 0.9 * n          # (an axis next to the marker's normal times a steep view: a tenth may hide below 2e-5)


def test_planted_translation_scale_fails():
    for name in ("fronto", "generic", "grazing", "far"):
        uv, q, (T1, e1, T2, e2) = oracle_on(name)
        Tb = T1.copy()
        Tb[:, :3, 3] = (Tb[:, :3, 3] * (1 + 1e-4)).astype(np.float32)
        assert _every_case_fails(q, Tb, e1, ec.family(name).resid_bar) == (ec.N, ec.N), name


def test_planted_swap_of_the_solutions_without_their_errors_fails():
    uv, q, (T1, e1, T2, e2) = oracle_on("oblique")
    assert (e2 - e1).min() > 1e-4
    assert _every_case_fails(q, T2, e1) == (ec.N, ec.N) and _every_case_fails(q, T1, e2) == (ec.N, ec.N)
