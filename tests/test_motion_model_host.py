"""The live tracker's motion model as the library runs it -- the C++ of host/motion_model.h, compiled here with the host compiler
(tests/tools/motion_main.cpp) -- against the mp reference tests/rotation_reference.py.  CPU only.  tests/test_live_motion_host.py holds the
model's Python restatement; nothing else runs the header itself without a GPU.

Cases: the pose's own rotation vector at every residual angle of tests/rotation_edge_cases.py (zero .. pi - 1e-12 and fl(pi n), |rvec| ~ pi
being the ordinary orientation of a board that faces the root camera) about every axis of the list (zero components, ties, a negative leading
component), with a zero motion, a motion of 1e-9 rad and one of ~0.03 rad.

    motion_between   wv against [log(R_a^T R_b) ; t_b - t_a]
    motion_apply     the result AS A ROTATION, |Exp(out) - R(z) Exp(w)| per entry (at a half turn the chart may pick either sign), |out| <= pi, t exact
    motion_measure   rel = s wv, pred as a rotation against R_b Exp(s log(R_a^T R_b)); the rule's zero cases (one frame, a gap over max_dt)
    motion_velocity, motion_predict   the same pieces with their own scalings

Bars: 8 x the float64 figures of rotation_edge_cases.F64_WORST (tests/test_rotation_reference_host.py measures them): a logarithm of R_a^T R_b at
small motions is the "between" site's e (8 x 2.4e-15), a logarithm of a product that lands anywhere up to pi is the "prior" site's (8 x 7.2e-15);
a result that is computed from another (pred from rel, predict from velocity) carries the sum of their bars, scaled as the formula scales them.

MEASURED, worst over the list.  While motion_so3_log called rodrigues_mat2vec near pi (the cv::Rodrigues restatement: theta from acos, and below
sin(theta) = 1e-5 the axis from the diagonal alone with OpenCV's sign rule):
    motion_apply 2.1e-6 at pi - 1e-6 (twice the distance to pi, as read from the code), and so motion_measure's prediction and motion_predict;
    motion_between 5.2e-16, rel 3.9e-16, velocity 1.3e-14 (the motions are small: their logarithm never reaches that branch)
With csrc/so3.hpp's near-pi branch in its place: motion_apply 1.1e-15, prediction 1.4e-15, motion_predict 1.4e-15 (bars 5.8e-14, 7.2e-14); the
others unchanged.
"""
import os
import subprocess

import numpy as np
import pytest

import rotation_edge_cases as ec
import rotation_reference as rr
from conftest import ROOT

M = rr.M
BETWEEN_BAR = ec.FACTOR * ec.F64_WORST["between"]["plain"]["e"]
LOG_BAR = ec.FACTOR * ec.F64_WORST["prior"]["plain"]["e"]
TA, TB, TIME = 0.0, 0.04, 0.07


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _cases():
    """(name, z [6] with the rotation vector theta n, motion (rvec, t) [6])"""
    rng = np.random.default_rng(2024)
    out = []
    for ia, th in enumerate(ec.RESIDUAL_ANGLES + ["nearest"]):
        for ix, ax in enumerate(ec.AXES):
            n = np.asarray(ax, dtype=np.float64) / np.linalg.norm(ax)
            w = ec.PI * n if th == "nearest" else th * n
            for tag, mag in (("zero", 0.0), ("tiny", 1e-9), ("small", 0.03 * (1 + rng.random()))):
                wv = np.r_[_unit(rng) * mag, (0.0 if mag == 0.0 else 1.0) * 0.02 * rng.standard_normal(3)]
                out.append(("a%s x%d %s" % (ia, ix, tag), np.r_[w, 0.3 * rng.standard_normal(3) + [0, 0, 3.0]], wv))
    return out


def _mp_mat_err(A, B):
    return float(max(abs(A[i][j] - B[i][j]) for i in range(3) for j in range(3)))


def _moved(z, wv):
    """the pose z moved by wv, rounded to float64: the second pose of a pair whose motion is (about) wv"""
    return np.r_[rr.partner_vector(z[:3], np.linalg.norm(wv[:3]), wv[:3], "own") if np.linalg.norm(wv[:3]) > 0 else z[:3], z[3:] + wv[3:]]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("motion")
    exe = str(tmp / "motion_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "tools", "motion_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    cases = _cases()
    recs = []
    for name, z, wv in cases:
        zb = _moved(z, wv)
        st = [2.0] + list(z) + list(zb) + [TA, TB]
        recs.append([0] + list(z) + list(zb))                 # between: the pose near the edge is end a ...
        recs.append([0] + list(zb) + list(z))                 # ... and end b
        recs.append([1] + list(z) + list(wv))                 # apply FROM the edge pose
        recs.append([1] + list(_moved(z, -wv)) + list(wv))    # apply ONTO the edge pose: the result is (about) z
        recs.append([2] + st + [TIME, 0.0])
        recs.append([3] + st)
        recs.append([4] + st + [TIME, 0.0])
    path = str(tmp / "in.txt")
    with open(path, "w") as f:
        for r in recs:
            f.write(" ".join(repr(float(v)) if i else str(int(v)) for i, v in enumerate(r)) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [np.array([float(v) for v in ln.split()]) for ln in run.stdout.strip().split("\n")]
    assert len(lines) == len(recs)
    return exe, tmp, cases, recs, lines


def _between_ref(za, zb):
    a, b = rr.mpv(za), rr.mpv(zb)
    return rr.between_e(a, b, None)


def test_motion_model_against_mp(results):
    _, _, cases, recs, lines = results
    worst = {}

    def see(key, name, v, bar):
        if v > worst.get(key, (-1, ""))[0]:
            worst[key] = (v, name, bar)

    over = []
    for n, (name, z, wv) in enumerate(cases):
        r = recs[7 * n:7 * n + 7]
        g = lines[7 * n:7 * n + 7]
        for k in (0, 1):
            za, zb = np.array(r[k][1:7]), np.array(r[k][7:13])
            ref = _between_ref(za, zb)
            see("between", name, max(abs(float(M.mpf(float(g[k][i])) - ref[i])) for i in range(6)), BETWEEN_BAR)
        for k in (2, 3):
            zz, ww = np.array(r[k][1:7]), np.array(r[k][7:13])
            Rref = rr.mat_mul(rr.exp(rr.mpv(zz[:3])), rr.exp(rr.mpv(ww[:3])))
            out = g[k]
            see("apply", name, _mp_mat_err(rr.exp(rr.mpv(out[:3])), Rref), LOG_BAR)
            assert np.linalg.norm(out[:3]) <= np.pi * (1 + 4e-16), (name, out)
            assert np.array_equal(out[3:], zz[3:] + ww[3:])
        za, zb = np.array(r[4][2:8]), np.array(r[4][8:14])
        wref = _between_ref(za, zb)
        s = (M.mpf(TIME) - M.mpf(TB)) / (M.mpf(TB) - M.mpf(TA))
        assert g[4][0] == 1.0
        rel, pred = g[4][1:7], g[4][7:13]
        see("measure rel", name, max(abs(float(M.mpf(float(rel[i])) - s * wref[i])) for i in range(6)), float(s) * BETWEEN_BAR + 2.0 ** -52 * 0.1)
        Rb = rr.exp(rr.mpv(zb[:3]))
        Rpred = rr.mat_mul(Rb, rr.exp([s * v for v in wref[:3]]))
        see("measure pred", name, _mp_mat_err(rr.exp(rr.mpv(pred[:3])), Rpred), LOG_BAR + float(s) * BETWEEN_BAR)
        assert np.abs(pred[3:] - (zb[3:] + rel[3:])).max() == 0.0
        dt = M.mpf(TB) - M.mpf(TA)
        see("velocity", name, max(abs(float(M.mpf(float(g[5][i])) - wref[i] / dt)) for i in range(6)), (BETWEEN_BAR + 2.0 ** -52 * 0.1) / float(dt))
        # predict: d * velocity, d / dt = s
        see("predict", name, _mp_mat_err(rr.exp(rr.mpv(g[6][:3])), Rpred), LOG_BAR + float(s) * (BETWEEN_BAR + 2.0 ** -52 * 0.1))
        see("predict t", name, float(max(abs(M.mpf(float(g[6][3 + i])) - (M.mpf(float(zb[3 + i])) + s * wref[3 + i])) for i in range(3))), 4 * 2.0 ** -52 * 4.0)
    for key, (v, name, bar) in sorted(worst.items()):
        print("MEASURED %-13s %.2e at %s (bar %.1e)" % (key, v, name, bar))
        if not v <= bar:
            over.append((key, v, name, bar))
    assert not over, over


def test_the_rule_of_motion_measure(results):
    """before two frames, and with a gap over max_dt, nothing is measured: rel is zero and the prediction is the newest pose bit for bit"""
    exe, tmp, cases, _, _ = results
    _, z, wv = cases[-1]
    zb = _moved(z, wv)
    recs = [[2, 1.0] + list(z) + list(zb) + [TA, TB, TIME, 0.0], [2, 2.0] + list(z) + list(zb) + [TA, TB, TIME, 0.02], [2, 2.0] + list(z) + list(zb) + [TA, TB, TIME, 0.035],
            [4, 2.0] + list(z) + list(zb) + [TA, TB, TIME, 0.02], [4, 2.0] + list(z) + list(zb) + [TA, TB, TB, 0.0], [3, 1.0] + list(z) + list(zb) + [TA, TB]]
    path = str(tmp / "rule.txt")
    with open(path, "w") as f:
        for r in recs:
            f.write(" ".join(repr(float(v)) if i else str(int(v)) for i, v in enumerate(r)) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    g = [np.array([float(v) for v in ln.split()]) for ln in run.stdout.strip().split("\n")]
    for k in (0, 1, 2):          # one frame; both gaps over 0.02; the older gap (0.04) over 0.035
        assert g[k][0] == 0.0 and not g[k][1:7].any() and np.array_equal(g[k][7:13], zb)
    assert np.array_equal(g[3], zb) and np.array_equal(g[4], zb)          # predict past max_dt, and at time == tb
    assert not g[5].any()
