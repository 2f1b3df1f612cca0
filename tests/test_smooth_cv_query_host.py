"""The numpy restatement of a constant-velocity smoothed track's pose and covariance at any time (tests/smooth_cv_query_restated.py, DESIGN.md
section 34) against the dense AUGMENTED system -- the frame inserted at the query's time and start pose, without detections -- on systems of
tests/smooth_cv_restated.py, the Gauss-Markov lag-three blocks, the changed-term lists, the claims of the definition, and the interface of
aar_track_smooth_query2 / aar_track_smooth_lag3 as header and binding declare it.  CPU only.

Yardstick: H' and g' - g from the restated system blocks of the augmented and the original data set, numpy.linalg.inv / solve.
Bars: cov: Frobenius error of the block over the Frobenius norm of the yardstick's block <= 10 eps kappa_2(H') (section 28's bar);
delta_m: error over |delta|_inf of the yardstick's full step <= max(10 eps kappa_2(H'), 1e-13) (section 31's floor).  The restatement takes
P = Sigma_NN from numpy's inverse of the original H and does the kernel's block algebra, so the cancellation in P^-1 - F_old is measured."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_cv_query_cases as cqc
import smooth_cv_query_restated as scq
import smooth_cv_restated as cv
import smooth_restated as sr
import track_restated as tr
from conftest import ROOT
from test_smooth_covariance_host import _base, _resized
from test_smooth_query_host import _times, _turned

EPS = np.finfo(np.float64).eps
SIG = (cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0)
ALPHAS = [1e-3, 0.1, 0.5, 0.9]
# frames without detections: smooth_cases.emptied (the first and the last frame from four frames on) and, at twelve, two neighbours and a
# single one inside, so that gaps lie beside and between emptied frames
EMPTY = {F: sorted(set(sc.emptied(F)) | ({4, 5, 8} if F == 12 else set())) for F in (1, 2, 3, 4, 5, 12)}


_PROBLEMS = {}


def _problem(F, uniform, step=0.3):
    """(ds, x, frame_time): x the SMOOTHED track (the restated LM run to convergence from the turned start), as a caller of the query holds
    it -- computed once, shared, not modified.  The yardstick forms g' - g from two full right-hand sides, so it is only as good as eps |g|:
    at a converged track g is rounding and g' - g is the changed terms' contribution to every digit"""
    if (F, uniform) not in _PROBLEMS:
        ds = sc.without_frames(_turned(_resized(_base("g_track_cfg2"), F), step), EMPTY[F])
        ft = _times(F, uniform)
        td = tr.TrackData(ds, np.array(ds.x_full))
        r = cv.smooth_lm(cv.SmoothCvProblem(td, *SIG, frame_time=ft), td.z0, min_avg=0.0, min_error=0.0, max_iters=60)
        n0 = sc.ns(ds)
        x = np.array(ds.x_full)
        x[n0:n0 + 6 * F] = r["z"].reshape(-1)
        _PROBLEMS[F, uniform] = (ds, x, ft, r["grad"])
    ds, x, ft, grad = _PROBLEMS[F, uniform]
    return ds, np.array(x), ft


def _system(ds, x, ft):
    td = tr.TrackData(ds, x)
    diag, off, off2, rhs = cv.SmoothCvProblem(td, *SIG, frame_time=ft).system(td.z0)
    return cv.dense(diag, off, off2), rhs


def _gaps(F):
    """the first, second, second-to-last and last gap (every subset of {a - 1, b + 1} is missing once over the sizes; a odd and a even) and
    the gaps beside / between emptied frames"""
    if F < 2:
        return []
    g = {0, 1, F - 3, F - 2} | {h for e in EMPTY[F] for h in (e - 1, e)}
    return sorted(h for h in g if 0 <= h <= F - 2)


def _queries(F, times):
    out = []
    for g in _gaps(F):
        for al in ALPHAS:
            out.append(("gap %d alpha %g" % (g, al), times[g] + al * (times[g + 1] - times[g])))
    sp = times[1] - times[0] if F > 1 else 1.0
    for d in (0.3, 4.0):
        out.append(("before %g" % d, times[0] - d * sp))
        out.append(("after %g" % d, times[-1] + d * (times[-1] - times[-2] if F > 1 else 1.0)))
    return out


WORST = {}


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 12])
def test_restated_query_against_the_dense_augmented_system(F, uniform):
    ds, x, ft = _problem(F, uniform)
    times = scq.times_of(F, ft)
    z = cqc.frames_of(ds, x)
    H, g = _system(ds, x, ft)
    Hinv = np.linalg.inv(H)
    if F >= 4:
        parity = {a % 2 for a in _gaps(F)}
        assert parity == {0, 1}
    wc, wd = 0.0, 0.0
    for tag, t in _queries(F, times):
        ds2, x2, ft2, pos = cqc.inserted(ds, x, ft, t)
        H2, g2 = _system(ds2, x2, ft2)
        want_cov, want_d, step, kappa = cqc.yardstick(H2, g2, g, pos)
        # g' - g is supported on the neighbours and m: exactly the changed terms' contribution
        _, _, nb = scq.changed_terms(F, times, t)
        d_full = (g2 - cqc.embedded(g, pos)).reshape(-1, 6)
        support = {f + (f >= pos) for f in nb} | {pos}
        assert len(support) <= 5
        for f in range(F + 1):
            if f not in support:
                assert np.abs(d_full[f]).max() <= 1e-9 * max(np.abs(g).max(), 1.0), (tag, f)
        pose, cov, seg, dm = scq.query(z, times, Hinv, t, SIG)
        assert seg == pos - 1 and np.array_equal(pose, scq.start_pose(z, times, t) + dm)
        e_c = np.linalg.norm(cov - want_cov) / np.linalg.norm(want_cov)
        e_d = np.abs(dm - want_d).max() / step if step > 0 else 0.0
        print("F %d %s %s: kappa %.2e, cov %.2e = %.4f eps kappa, delta %.2e = %.4f eps kappa (|step| %.2e)" %
              (F, "uniform" if uniform else "uneven", tag, kappa, e_c, e_c / (EPS * kappa), e_d, e_d / (EPS * kappa), step))
        assert e_c <= 10 * EPS * kappa, (tag, e_c, EPS * kappa)
        if tag.startswith("after") and F > 1:
            # the one case dropped from the step's bar: nothing is removed and the new term is zero at the start pose,
            # so g' - g and the yardstick's whole step are rounding (1e-16) and a quotient of the two says nothing.  What holds instead is the
            # definition's own statement, the pose is the extrapolation to rounding: the term is below 1e-15 at the start pose and its
            # Jacobian in m is J_r(phi)^-1 J_l(w_m)^T, conditioned below 10 at these angles
            assert step <= 1e-14 and np.abs(dm).max() <= 1e-14, (tag, step, dm)
            e_d = 0.0
        assert e_d <= max(10 * EPS * kappa, 1e-13), (tag, e_d, EPS * kappa)
        wc, wd = max(wc, e_c / (EPS * kappa)), max(wd, e_d / (EPS * kappa))
        assert np.array_equal(cqc.frames_of(ds2, x2)[pos], scq.start_pose(z, times, t))
    WORST[(F, uniform)] = (wc, wd)
    print("F %d: the largest errors are %.4f (cov) and %.4f (delta) eps kappa_2(H')" % (F, wc, wd))


@pytest.mark.parametrize("F", [4, 5, 6, 9])
def test_gauss_markov_lag_three_against_the_dense_inverse(F):
    ds = sc.without_frames(_turned(_resized(_base("g_track_cfg2"), F), 0.3), sc.emptied(F))
    H, _ = _system(ds, np.array(ds.x_full), _times(F, False))
    kappa = np.linalg.cond(H)
    Hinv = np.linalg.inv(H)
    S, R = scq.supernode_blocks(Hinv, F)
    l3 = scq.gauss_markov_lag3(S, R, F)
    assert l3.shape == (F - 3, 6, 6)
    for f in range(F - 3):
        want = Hinv[6 * f:6 * f + 6, 6 * f + 18:6 * f + 24]
        e = np.linalg.norm(l3[f] - want) / np.linalg.norm(want)
        print("F %d f %d: kappa %.2e, lag three %.2e = %.4f eps kappa" % (F, f, kappa, e, e / (EPS * kappa)))
        assert e <= 10 * EPS * kappa, (f, e)


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 12])
def test_changed_terms_against_the_model_of_the_augmented_times(F):
    times = scq.times_of(F, _times(F, False))
    old = set(scq.model_terms(F))
    for tag, t in _queries(F, times):
        rem, add, nb = scq.changed_terms(F, times, t)
        pos = scq.locate(times, t)[0] + 1
        up = lambda fr: tuple(pos if f == "m" else f + (f >= pos) for f in fr)
        new = set(scq.model_terms(F + 1))
        kept = {up(fr) for fr in old - set(rem)}
        assert set(rem) <= old and len(set(rem)) == len(rem), tag
        assert kept | {up(fr) for fr in add} == new and not kept & {up(fr) for fr in add}, (tag, rem, add)
        assert len(rem) <= 2 + (pos == 1 and F > 1) and len(add) <= 3 + (pos <= 1), tag
        touched = {f for fr in rem + add for f in fr if f != "m"}
        assert touched <= set(nb) and nb == sorted(nb) and len(nb) <= 4, tag


@pytest.mark.parametrize("F", [2, 3, 12])
def test_the_new_term_is_zero_at_the_start_pose_outside(F):
    # 1e-15 is 4.5 eps: the start pose is stored as a rotation vector, rounded to eps |w_m|, and the term expands it again and multiplies three
    # rotation matrices (3 eps / 2 an entry each).  That fits below 1e-15 while |w| stays below 2 rad -- config 2's own first frames (1.7 rad),
    # inter-frame rotations as recorded and of 0.1 rad; on the turned and smoothed twelve-frame track of _problem (2.3 rad) the same term
    # measures 1.25e-15, which is the number format's doing and not a property of the start pose
    for step in (0.0, 0.1):
        ds = _turned(_resized(_base("g_track_cfg2"), F), step)
        ft = _times(F, False)
        times = scq.times_of(F, ft)
        z = cqc.frames_of(ds, np.array(ds.x_full))
        assert np.linalg.norm(z[:, :3], axis=1).max() < 2.0
        _zero_outside(F, z, times)


def _zero_outside(F, z, times):
    for d in (0.3, 4.0):
        t = times[-1] + d * (times[-1] - times[-2])
        zm = scq.start_pose(z, times, t)
        e = cv.cv_term(z[F - 2], z[F - 1], zm, (t - times[-1]) / (times[-1] - times[-2]))
        assert np.abs(e).max() <= 1e-15, (F, d, e)
        t = times[0] - d * (times[1] - times[0])
        zm = scq.start_pose(z, times, t)
        e = cv.cv_term(zm, z[0], z[1], (times[1] - times[0]) / (times[0] - t))
        assert np.abs(e).max() <= 1e-15, (F, d, e)


def test_on_a_frame_time():
    ds, x, ft = _problem(12, False)
    times = scq.times_of(12, ft)
    z = cqc.frames_of(ds, x)
    Hinv = np.linalg.inv(_system(ds, x, ft)[0])
    for f in (0, 5, 11):
        pose, cov, seg, _ = scq.query(z, times, Hinv, times[f], SIG)
        assert seg == f and np.array_equal(pose, z[f]) and np.array_equal(cov, Hinv[6 * f:6 * f + 6, 6 * f:6 * f + 6])


# ---- the claims of the definition ----
def _converged(ds2, x2, ft2, sig=SIG, **lm):
    td = tr.TrackData(ds2, x2)
    return cv.smooth_lm(cv.SmoothCvProblem(td, *sig, frame_time=ft2), td.z0, **lm)


def _rot_dist(za, zb):
    return float(np.linalg.norm(sr.between(za, zb)))


CLAIM_LM = dict(min_avg=0.0, max_iters=40)      # both runs stop by themselves after about twenty iterations, gradient 1e-8


def test_claim_one_step_reaches_the_augmented_minimiser():
    # section 31's claim case: config 2, frames {0, 99, 33 .. 42} emptied, smoothed to convergence; queries in the gap beside the emptied first
    # frame, the gap before the emptied run and a gap inside it.  The distance of the query's pose to the converged z_m of the augmented
    # problem over the distance of the start pose to it.  Measured here: 0.003, 0.005 and 0.0001 -- inside the run the
    # geodesic is 1.6e-3 away and one step lands within 2e-7.  The worst is below 0.25, so the bar is 0.5, section 31's rule.  (At section
    # 31's fourteen iterations neither run has converged inside the run -- gradient 1e-2 -- and the quotient there measures the LM, not the
    # step: 0.87.  Hence the longer runs.)
    ds, x0, empty = cc.claim_case()
    F = ds.num_frames
    td = tr.TrackData(ds, x0)
    r = cv.smooth_lm(cv.SmoothCvProblem(td, *SIG), td.z0, **CLAIM_LM)
    assert r["iterations"] < 40
    z = r["z"]
    n0 = sc.ns(ds)
    x = np.concatenate([x0[:n0], z.reshape(-1), x0[n0 + 6 * F:]])
    times = scq.times_of(F, None)
    H, _ = _system(ds, x, None)
    Hinv = np.linalg.inv(H)
    worst = 0.0
    for t in (0.5, 32.5, 37.25):
        pose, _, _, _ = scq.query(z, times, Hinv, t, SIG)
        ds2, x2, ft2, pos = cqc.inserted(ds, x, None, t)
        r2 = _converged(ds2, x2, ft2, **CLAIM_LM)
        assert r2["iterations"] < 40
        zc, z0m = r2["z"][pos], scq.start_pose(z, times, t)
        d1, d0 = _rot_dist(pose, zc), _rot_dist(z0m, zc)
        print("claim t %.2f: |query - converged| %.3e, |start - converged| %.3e, ratio %.4f" % (t, d1, d0, d1 / d0))
        worst = max(worst, d1 / d0)
    assert worst <= 0.5, worst


def test_noiseless_constant_motion_is_returned_at_any_time():
    ds, x0, zt, ft, empty, _ = cc.constant_velocity_sequence()
    F = len(ft)
    td = tr.TrackData(ds, x0)
    sig = (1e-3, 1e-3, 1e3, 1e3)
    r = cv.smooth_lm(cv.SmoothCvProblem(td, *sig, frame_time=ft), td.z0, min_avg=0.0, min_error=0.0, max_iters=100)
    z = r["z"]
    n0 = sc.ns(ds)
    x = np.concatenate([x0[:n0], z.reshape(-1)])
    Hinv = np.linalg.inv(_system_sig(ds, x, ft, sig))
    w, v = np.array([0.02, -0.025, 0.03]), np.array([0.004, -0.002, 0.003])
    R0 = tr.rodrigues(zt[0][:3])
    worst = 0.0
    for t in (ft[0] - 0.3, ft[0] - 4.0, ft[0] + 0.4, ft[5] + 0.5 * (ft[6] - ft[5]), ft[6] + 1e-3, ft[-2] + 0.9 * (ft[-1] - ft[-2]), ft[-1] + 0.3,
              ft[-1] + 4.0):
        pose, cov, _, _ = scq.query(z, ft, Hinv, t, sig)
        truth = np.r_[sr.so3_log(R0 @ tr.rodrigues((t - ft[0]) * w)), zt[0][3:] + (t - ft[0]) * v]
        worst = max(worst, np.abs(pose - truth).max())
        print("constant motion t %.4f: error %.2e" % (t, np.abs(pose - truth).max()))
        assert np.linalg.eigvalsh(cov)[0] > 0
    assert worst < 1e-7, worst


def _system_sig(ds, x, ft, sig):
    td = tr.TrackData(ds, x)
    diag, off, off2, _ = cv.SmoothCvProblem(td, *sig, frame_time=ft).system(td.z0)
    return cv.dense(diag, off, off2)


def test_pure_translation_is_exact():
    # an object that only translates, on a path that is NOT of constant velocity, noiseless: every rotation term of the prior sits at zero and
    # the translation rows are linear, so one step lands on m's component of the augmented minimiser (1e-9: the poses' bar of section 31)
    ds, x0, zt, ft, empty = cqc.translating_sequence()
    F = len(ft)
    n0 = sc.ns(ds)
    lm = dict(min_avg=0.0, min_error=0.0, max_iters=100)
    r = _converged(ds, x0, ft, **lm)
    z = r["z"]
    assert np.abs(z[:, :3] - zt[:, :3]).max() < 1e-3 and np.abs(np.diff(zt[:, 3:], 2, axis=0)).max() > 1e-3
    x = np.concatenate([x0[:n0], z.reshape(-1)])
    Hinv = np.linalg.inv(_system(ds, x, ft)[0])
    for t in (ft[0] - 0.7, ft[0] + 0.3, ft[F // 2] - 0.5, ft[-2] + 0.9 * (ft[-1] - ft[-2]), ft[-1] + 2.0):
        pose, _, _, _ = scq.query(z, ft, Hinv, t, SIG)
        ds2, x2, ft2, pos = cqc.inserted(ds, x, ft, t)
        r2 = _converged(ds2, x2, ft2, **lm)
        e = np.abs(pose - r2["z"][pos]).max()
        print("translations t %.3f: |query - converged| %.2e (the start pose: %.2e)" % (t, e, np.abs(scq.start_pose(z, ft, t) - r2["z"][pos]).max()))
        assert e <= 1e-9, (t, e)


# ---- the interface ----
def _refused(word, *a, **kw):
    with pytest.raises(aar.AarError) as e:
        aar.smooth_query_validate(*a, **kw)
    assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), str(e.value)


CV = dict(model="cv", sigma_rot0=1.0, sigma_trans0=1.0)


def test_validate_under_the_model():
    aar.smooth_query_validate(5, cc.SROT, cc.STRANS, [0.5, -3.0, 17.0, 0.5], **CV)
    aar.smooth_query_validate(0, cc.SROT, cc.STRANS, [], **CV)
    aar.smooth_query_validate(1, cc.SROT, cc.STRANS, [2.0], frame_time=[1.0], **CV)
    _refused("query_time[2]", 5, cc.SROT, cc.STRANS, [0.0, 1.0, np.nan], **CV)
    _refused("num_frames", 0, cc.SROT, cc.STRANS, [0.0], **CV)
    _refused("sigma_rot0", 5, cc.SROT, cc.STRANS, [0.0], model="cv", sigma_rot0=-1.0, sigma_trans0=1.0)
    _refused("sigma_trans0", 5, cc.SROT, cc.STRANS, [0.0], model="cv", sigma_rot0=1.0, sigma_trans0=0.0)
    _refused("rel_motion", 3, cc.SROT, cc.STRANS, [0.0], rel_motion=np.zeros((2, 6)), **CV)
    _refused("frame_time[2]", 3, cc.SROT, cc.STRANS, [0.0], frame_time=[0.0, 1.0, 1.0], **CV)


def test_header_and_binding_declare_the_calls():
    with open(os.path.join(ROOT, "include", "aar.h")) as f:
        h = f.read()
    for n in ("aar_track_smooth_query2", "aar_track_smooth_lag3"):
        assert re.search(r"\bint\s+%s\s*\(" % n, h), n
        assert n in aar.SYMBOLS and hasattr(aar.lib(), n), n
    assert hasattr(aar.Problem, "track_smooth_query2") and hasattr(aar.Problem, "track_smooth_lag3")
    assert C.sizeof(aar.CSmoothQueryReport) == 80
