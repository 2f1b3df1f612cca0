"""The constant-velocity smoothed track at any time (aar_track_smooth_query2, aar_track_smooth_lag3): pose and covariance
block at query times between, on and outside the frame times.  Needs a real MI355X.

The answer at a time t is what one Gauss-Newton step of the constant-velocity smoother reports for a frame m without detections inserted at t,
so the yardstick is the dense AUGMENTED system on the device's own blocks: H' and g' from aar_track_smooth_system2 on the augmented data set
(tests/smooth_cv_query_cases.inserted, m at the start pose the device reports), g from the same call on the original one, solved with
numpy.linalg.inv / solve.  Bars: cov: Frobenius error of the block over the Frobenius norm of the yardstick's block <= 10 eps kappa_2(H');
delta_m (aar_track_smooth_query2_step: the pose itself carries the step only to eps |z_m|): error over |delta|_inf of the yardstick's full step
<= max(10 eps kappa_2(H'), 1e-13).  Where the exact step is zero -- after the end, and in the last gap before a last frame without detections
-- the step has no such bar: g' - g is rounding there (_hold says why) and |delta_m| <= 1e-13 is held instead.  x_full is the SMOOTHED track,
as a caller holds it: the yardstick's g' - g is a difference of two full right-hand sides and only as good as eps |g|.
"""
import ctypes as C
import os
import subprocess

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
from conftest import PKG, ROOT, load_golden
from test_gpu_track_smooth_query import parse_resampled_yaml

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SROT, STRANS = cc.SROT, cc.STRANS
CV = dict(model="cv", sigma_rot0=cc.SROT0, sigma_trans0=cc.STRANS0)
T = 16                       # SMOOTH_CV_T of csrc/kernels.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _lm():
    return aar.lm_default_params(min_average_step_error_diff=0.0, max_iters=40)


def _dataset(F):
    """config 2 cut to F frames with the frames of sc.emptied(F) emptied"""
    ds = sc.without_frames(aar.synth(2, num_frames=F), sc.emptied(F))
    assert ds.num_frames == F
    return ds


def _frame_time(F):
    return 0.25 + cc.gaps(F) if F > 1 else None


def _problem(ds, delta=None):
    p = aar.Problem(ds, with_huber=delta is not None)
    if delta is not None:
        p.set_huber_delta(delta)
    return p


def _gaps_of(F):
    """the gaps queried: the first and the last; at 65 frames (sc.emptied: 0, 21 .. 30, 64; supernode k = frames 2k, 2k + 1) 0 beside the emptied
    first frame, 20 beside the emptied run (a even: a - 1 odd, its lag-three block by the Gauss-Markov product), 25 between emptied frames (a
    odd), 40 and 61 between observed frames (even, odd), 63 = frames 63 | 64 across supernodes 31 | 32 and beside the emptied last frame"""
    if F < 2:
        return []
    return sorted({0, F - 2} | ({20, 25, 40, 61} if F == 65 else set()))


def _query_times(F, times):
    out = []
    for g in _gaps_of(F):
        for al in (1e-3, 0.5):
            out.append(times[g] + al * (times[g + 1] - times[g]))
    return np.array(out + [times[0] - 0.3, times[-1] + 4.0])


def _rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


_CASES = {}


def _case(F, delta=None, ds=None):
    """the smoothed track of one shape, its query call and, per query, the yardstick from the augmented data set -- computed once, shared, not
    modified"""
    key = (F, delta, ds is None)
    if key in _CASES:
        return _CASES[key]
    if ds is None:
        ds = _dataset(F)
        x0, ft = sc.track_start(ds), _frame_time(F)
    else:
        x0, ft = np.array(ds.x_full), None
    assert ds.num_frames == F
    times = scq.times_of(F, ft)
    qt = _query_times(F, times)
    with _problem(ds, delta) as p:
        x = p.track_smooth(x0, SROT, STRANS, frame_time=ft, params=_lm(), **CV)[0]
        pose, cov, seg, rep = p.track_smooth_query2(x, SROT, STRANS, qt, frame_time=ft, **CV)
        pose_only, none, seg_only, rep_only = p.track_smooth_query2(x, SROT, STRANS, qt, frame_time=ft, covariance=False, **CV)
        start, step = p.track_smooth_query2_step(x, SROT, STRANS, qt, frame_time=ft, **CV)
        S, R, R2, crep = p.track_smooth_covariance2(x, SROT, STRANS, frame_time=ft, **CV)
        g = p.track_smooth_system2(x, SROT, STRANS, 0.0, frame_time=ft, **CV)[3]
    assert none is None
    yard = []
    for k, t in enumerate(qt):
        ds2, x2, ft2, pos = cqc.inserted(ds, x, ft, t, zm=start[k])
        with _problem(ds2, delta) as p:
            gd, go, go2, g2, _, _ = p.track_smooth_system2(x2, SROT, STRANS, 0.0, frame_time=ft2, **CV)
        yard.append(cqc.yardstick(cv.dense(gd, go, go2), g2, g, pos))
    out = dict(ds=ds, x=x, ft=ft, times=times, qt=qt, pose=pose, cov=cov, seg=seg, rep=rep, pose_only=pose_only, seg_only=seg_only,
               rep_only=rep_only, start=start, step=step, S=S, crep=crep, yard=yard,
               free_end=not np.any(np.asarray(ds.obs_frame) == F - 1))
    _CASES[key] = out
    return out


def _hold(tag, c):
    F = len(c["times"])
    wc = wd = 0.0
    for k, t in enumerate(c["qt"]):
        want_cov, want_d, full, kappa = c["yard"][k]
        a, kind = scq.locate(c["times"], t)
        assert c["seg"][k] == a
        e_c = _rel(c["cov"][k], want_cov)
        e_d = float(np.abs(c["step"][k] - want_d).max() / full) if full > 0 else 0.0
        print("%s t %.6g (%s, segment %d): kappa %.3e, cov %.2e = %.4f eps kappa, delta %.2e = %.4f eps kappa (|step| %.2e)" %
              (tag, t, kind, a, kappa, e_c, e_c / (EPS * kappa), e_d, e_d / (EPS * kappa), full))
        assert e_c <= 10 * EPS * kappa, (t, e_c, 10 * EPS * kappa)
        if (kind == "after" and F > 1) or (kind == "inside" and a == F - 2 and F >= 3 and c["free_end"]):
            # dropped from the step's bar: the exact step is ZERO.  After the end nothing is removed and the new term vanishes at the start
            # pose; in the last gap before a last frame without detections that frame sits on the extrapolation of the two before it (its one
            # term is zero at the smoothed track), and so does m on the geodesic.  g' - g and the yardstick's whole step are rounding and a
            # quotient of two roundings says nothing; what is held is that the step is rounding: the terms' own, eps (1 + r) |z|, through a
            # Jacobian of size 1 + r
            assert np.abs(c["step"][k]).max() <= 1e-13, (t, full, c["step"][k])
        else:
            assert e_d <= max(10 * EPS * kappa, 1e-13), (t, e_d, 10 * EPS * kappa)
            wd = max(wd, e_d / (EPS * kappa))
        wc = max(wc, e_c / (EPS * kappa))
        # the start pose is the restated one, and the pose is the sum of the two summands to the bit
        assert np.abs(c["start"][k] - scq.start_pose(cqc.frames_of(c["ds"], c["x"]), c["times"], t)).max() <= 1e-12
        assert np.array_equal(c["pose"][k], c["start"][k] + c["step"][k])
    print("%s: largest %.4f (cov) and %.4f (delta) eps kappa_2(H')" % (tag, wc, wd))


def _own_levels(F):
    K, n, s = (F + 1) // 2, 0, 1
    while s < K and -(-K // (2 * s)) > T:
        n, s = n + 1, 2 * s
    return n


# ---- 1. covariance and step against the dense augmented system ----
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 65])
def test_query_against_the_dense_augmented_system(F):
    c = _case(F)
    _hold("F %d" % F, c)
    assert np.all(np.isfinite(c["cov"])) and min(np.linalg.eigvalsh(m)[0] for m in c["cov"]) > 0
    assert np.array_equal(c["cov"], np.swapaxes(c["cov"], 1, 2))
    n_in = 2 * len(_gaps_of(F))
    rep = c["rep"]
    assert (rep["num_queries"], rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (n_in + 2, n_in, 0, 2)
    # the chain of aar_track_smooth_covariance2, the lag-three kernel from four frames on, the queries
    assert rep["launches"] == c["crep"]["launches"] + (F >= 4) + 1
    for k in ("num_residuals", "num_vars", "data_cost", "prior_cost", "sigma2"):
        assert rep[k] == c["crep"][k], k
    # cov = NULL: the same chain, the same poses
    assert np.array_equal(c["pose_only"], c["pose"]) and np.array_equal(c["seg_only"], c["seg"])
    assert c["rep_only"]["launches"] == rep["launches"] and c["rep_only"]["sigma2"] == rep["sigma2"]
    assert _own_levels(65) == 1 and _own_levels(64) == 0


# ---- 2. the lag-three blocks ----
@pytest.mark.parametrize("F", [4, 5, 6, 65])
def test_lag3_against_the_dense_inverse(F):
    ds = _dataset(F)
    x0, ft = sc.track_start(ds), _frame_time(F)
    with aar.Problem(ds) as p:
        gd, go, go2, _, _, _ = p.track_smooth_system2(x0, SROT, STRANS, 0.0, frame_time=ft, **CV)
        l3 = p.track_smooth_lag3(x0, SROT, STRANS, frame_time=ft, **CV)
        l3b = p.track_smooth_lag3(x0, SROT, STRANS, frame_time=ft, **CV)
    H = cv.dense(gd, go, go2)
    ev = np.linalg.eigvalsh(H)
    kappa = float(ev[-1] / ev[0])
    Hi = np.linalg.inv(H)
    assert l3.shape == (F - 3, 6, 6) and np.array_equal(l3, l3b)
    worst = 0.0
    for f in range(F - 3):
        e = _rel(l3[f], Hi[6 * f:6 * f + 6, 6 * f + 18:6 * f + 24])
        worst = max(worst, e)
        assert e <= 10 * EPS * kappa, (f, e, 10 * EPS * kappa)
    print("F %d: kappa %.3e, lag three: largest %.2e = %.4f eps kappa" % (F, kappa, worst, worst / (EPS * kappa)))


def test_lag3_small_sizes_and_the_random_walk():
    ds = _dataset(3)
    with aar.Problem(ds) as p:
        l3 = np.full((2, 36), 7.0)
        x = np.array(p._x(sc.track_start(ds)), dtype=np.float64)
        sp = aar.SmoothParams(SROT, STRANS, None, None, None, **CV)
        assert aar.lib().aar_track_smooth_lag3(p.handle, aar._dptr(x), C.byref(sp.c), aar._dptr(l3)) == 0 and np.all(l3 == 7.0)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_lag3(sc.track_start(ds), SROT, STRANS, model="rw")
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_query2_step(sc.track_start(ds), SROT, STRANS, [0.5], model="rw")
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED


# ---- 3. a Huber problem ----
def _golden_track(name):
    ds, g = load_golden(name)
    ds.x_full = np.array(g["track_x0"])
    return ds


def test_huber_problem():
    ds = _golden_track("g_track_cfg2_huber")
    F = ds.num_frames
    assert F >= 3
    c = _case(F, 1.0, ds=ds)
    _hold("huber", c)
    with aar.Problem(ds) as p:
        plain = p.track_smooth_query2(c["x"], SROT, STRANS, c["qt"], **CV)[1]
    # the weights are in the blocks: down-weighted detections leave the poses less certain
    assert np.einsum("qii->", c["cov"]) > np.einsum("qii->", plain)


# ---- 4. on a frame time ----
@pytest.mark.parametrize("F", [1, 3, 65])
def test_on_a_frame_time(F):
    c = _case(F)
    z = cqc.frames_of(c["ds"], c["x"])
    with aar.Problem(c["ds"]) as p:
        pose, cov, seg, rep = p.track_smooth_query2(c["x"], SROT, STRANS, c["times"], frame_time=c["ft"], **CV)
    assert np.array_equal(pose, z) and np.array_equal(cov, c["S"]) and np.array_equal(seg, np.arange(F))
    assert (rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (0, F, 0)


# ---- 5. shapes and bits ----
def _mixed_times(times, Q, seed):
    """Q query times: inside, on frames, outside, with duplicates, shuffled"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(times[0] - 2.0, times[-1] + 2.0, size=Q)
    t[::5] = rng.choice(times, size=len(t[::5]))              # on frame times
    if Q >= 5:
        t[3] = t[1]                                           # a duplicate
    if Q >= 8:
        t[3::7] = t[1]
    rng.shuffle(t)
    return t


@pytest.mark.parametrize("Q", [0, 1, 4, 5, 257])
def test_shapes_and_bits(Q):
    c = _case(65)
    ds, x, ft, times = c["ds"], c["x"], c["ft"], c["times"]
    qt = _mixed_times(times, Q, 5 + Q)
    keep = np.array(x)
    with aar.Problem(ds) as p:
        pose, cov, seg, rep = p.track_smooth_query2(x, SROT, STRANS, qt, frame_time=ft, **CV)
        pose2, cov2, seg2, rep2 = p.track_smooth_query2(x, SROT, STRANS, qt, frame_time=ft, **CV)
        pose3, none, seg3, _ = p.track_smooth_query2(x, SROT, STRANS, qt, frame_time=ft, covariance=False, **CV)
        alone = {t: p.track_smooth_query2(x, SROT, STRANS, [t], frame_time=ft, **CV) for t in np.unique(qt)}
    assert np.array_equal(x, keep) and none is None
    assert pose.shape == (Q, 6) and cov.shape == (Q, 6, 6) and seg.shape == (Q,)
    assert np.array_equal(pose, pose2) and np.array_equal(cov, cov2) and np.array_equal(seg, seg2)       # two calls: identical
    assert np.array_equal(pose, pose3) and np.array_equal(seg, seg3)                                     # cov = NULL: the same poses
    kinds = [scq.locate(times, t) for t in qt]
    for k, t in enumerate(qt):
        p1, c1, s1, _ = alone[t]
        assert pose[k].tobytes() == p1[0].tobytes() and cov[k].tobytes() == c1[0].tobytes() and seg[k] == s1[0] == kinds[k][0], (k, t)
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))                                                   # symmetric to the bit
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(pose))
    assert all(np.linalg.eigvalsh(m)[0] > 0 for m in cov)
    count = [sum(kd == w for _, kd in kinds) for w in ("inside", "on")]
    assert (rep["num_queries"], rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (Q, count[0], count[1], Q - sum(count))
    if Q >= 257:
        assert min(count) > 0 and Q - sum(count) > 0 and len(np.unique(qt)) < Q
    assert rep["launches"] == (c["crep"]["launches"] + 2 if Q else 0)


# ---- 6. nothing else moves ----
def test_nothing_else_moves():
    c = _case(65)
    ds, ft, times = c["ds"], c["ft"], c["times"]
    x0 = sc.track_start(ds)
    qt = _mixed_times(times, 9, 3)
    with aar.Problem(ds) as p:
        a0 = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
        b0 = p.track_smooth_covariance2(a0[0], SROT, STRANS, frame_time=ft, **CV)
        p.track_smooth_query2(a0[0], SROT, STRANS, qt, frame_time=ft, **CV)
        p.track_smooth_lag3(a0[0], SROT, STRANS, frame_time=ft, **CV)
        a1 = p.track_smooth(x0, SROT, STRANS, frame_time=ft, **CV)
        b1 = p.track_smooth_covariance2(a0[0], SROT, STRANS, frame_time=ft, **CV)
        # the random walk through the new entry is the old entry
        r0 = p.track_smooth_query(a0[0], SROT, STRANS, qt, frame_time=ft)
        r1 = p.track_smooth_query2(a0[0], SROT, STRANS, qt, frame_time=ft)
        r2 = p.track_smooth_query2(a0[0], SROT, STRANS, qt, frame_time=ft, model="rw")
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_query(a0[0], SROT, STRANS, qt, frame_time=ft, **CV)
        assert e.value.code == aar.AAR_ERR_UNSUPPORTED and "aar_track_smooth_query2" in str(e.value)
    for got, want in ((a1, a0), (b1, b0), (r1, r0), (r2, r0)):
        for u, v in zip(got, want):
            if isinstance(u, dict):
                assert all(k == "seconds" or u[k] == v[k] for k in u)
            else:
                assert np.array_equal(u, v)


# ---- 7. refusals ----
def _last_error():
    return aar.lib().aar_last_error().decode("utf-8", "replace")


def _raw(p, x0, qt, ft=None, pose=True, cov=True, seg=True, report=True, struct_size=None, fill=7.0):
    x = np.array(p._x(x0), dtype=np.float64)
    keep = x.copy()
    spar = aar.SmoothParams(SROT, STRANS, ft, None, None, **CV)
    qt = np.ascontiguousarray(qt, dtype=np.float64)
    Q = len(qt)
    po, co, sg = np.full((max(Q, 1), 6), fill), np.full((max(Q, 1), 36), fill), np.full(max(Q, 1), 77, dtype=np.int32)
    rep = aar.CSmoothQueryReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep) if struct_size is None else struct_size
    code = aar.lib().aar_track_smooth_query2(p.handle, aar._dptr(x), C.byref(spar.c), Q, aar._dptr(qt), aar._dptr(po) if pose else None,
                                             aar._dptr(co) if cov else None, sg.ctypes.data_as(C.POINTER(C.c_int32)) if seg else None,
                                             C.byref(rep) if report else None)
    assert np.array_equal(x, keep)
    return code, po, co, sg, rep


def _untouched(rep):
    return bytes(bytearray(rep)[4:]) == b"\x55" * (C.sizeof(rep) - 4)


def test_refusals():
    c = _case(5)
    ds, x, ft = c["ds"], c["x"], c["ft"]
    t = c["times"]
    ok = [t[0] + 0.5, t[1], t[-1] + 9.0]
    with aar.Problem(ds) as p:
        code, po, co, sg, rep = _raw(p, x, [t[0] + 0.5, t[1], t[0], np.nan, 2.0], ft)
        assert code == aar.AAR_ERR_INVALID and "query_time[3]" in _last_error()
        assert np.all(po == 7.0) and np.all(co == 7.0) and np.all(sg == 77) and _untouched(rep)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_query2(x, SROT, STRANS, [0.5], model="cv", sigma_rot0=-1.0, sigma_trans0=1.0)
        assert e.value.code == aar.AAR_ERR_INVALID and "sigma_rot0" in str(e.value)
        # NULL outputs in every combination and a caller compiled against a shorter report
        code, po, co, sg, rep = _raw(p, x, ok, ft)
        assert code == 0 and not np.any(po == 7.0) and not np.any(co == 7.0) and list(sg) == [0, 1, 4]
        for mask in range(16):
            kw = dict(pose=bool(mask & 1), cov=bool(mask & 2), seg=bool(mask & 4), report=bool(mask & 8))
            code, po2, co2, sg2, rep2 = _raw(p, x, ok, ft, **kw)
            assert code == 0, kw
            assert np.array_equal(po2, po) if kw["pose"] else np.all(po2 == 7.0)
            assert np.array_equal(co2, co) if kw["cov"] else np.all(co2 == 7.0)
            assert np.array_equal(sg2, sg) if kw["seg"] else np.all(sg2 == 77)
            assert (rep2.sigma2 == rep.sigma2 and rep2.num_outside == 1) if kw["report"] else _untouched(rep2)
        cut = aar.CSmoothQueryReport.num_queries.offset
        code, _, _, _, rep3 = _raw(p, x, ok, ft, struct_size=cut)
        assert code == 0 and rep3.struct_size == cut and rep3.sigma2 == rep.sigma2 and rep3.num_vars == 30
        assert bytes(bytearray(rep3)[cut:]) == b"\x55" * (C.sizeof(rep3) - cut)
    nothing = sc.without_frames(aar.synth(2, num_frames=6), range(6))                  # a recording without any detection
    assert nothing.num_obs == 0
    with aar.Problem(nothing) as p:
        for kw in (dict(), dict(cov=False)):                                           # the pose needs the block: no poses without it either
            code, po, co, sg, rep = _raw(p, sc.track_start(nothing), [0.5, 2.0, -1.0], **kw)
            assert code == aar.AAR_ERR_NUMERIC and np.all(po == 7.0) and np.all(co == 7.0) and np.all(sg == 77) and _untouched(rep)


def test_unsupported_behind_a_communicator():
    ds = _golden_track("g_track_cfg2")
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            code, po, co, sg, rep = _raw(p, ds.x_full, [0.5])
            assert code == aar.AAR_ERR_UNSUPPORTED and np.all(po == 7.0) and np.all(co == 7.0) and np.all(sg == 77) and _untouched(rep)
            with pytest.raises(aar.AarError) as e:
                p.track_smooth_lag3(ds.x_full, SROT, STRANS, **CV)
            assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    finally:
        comm.close()
        group.close()


# ---- 8. the claims, on the cases of tests/test_smooth_cv_query_host.py ----
def _smoothed(ds, x0, ft, sig, **lm):
    with aar.Problem(ds) as p:
        return p.track_smooth(x0, sig[0], sig[1], frame_time=ft, params=aar.lm_default_params(**lm), model="cv", sigma_rot0=sig[2], sigma_trans0=sig[3])[0]


def test_claim_one_step_reaches_the_augmented_minimiser():
    # measured on the CPU (tests/test_smooth_cv_query_host.py): 0.003, 0.005, 0.0001; below 0.25, so the bar is 0.5, section 31's rule
    ds, x0, empty = cc.claim_case()
    F = ds.num_frames
    sig = (SROT, STRANS, cc.SROT0, cc.STRANS0)
    lm = dict(min_average_step_error_diff=0.0, max_iters=40)
    x = _smoothed(ds, x0, None, sig, **lm)
    times = scq.times_of(F, None)
    qt = [0.5, 32.5, 37.25]
    with aar.Problem(ds) as p:
        pose = p.track_smooth_query2(x, SROT, STRANS, qt, **CV)[0]
        start = p.track_smooth_query2_step(x, SROT, STRANS, qt, **CV)[0]
    for k, t in enumerate(qt):
        ds2, x2, ft2, pos = cqc.inserted(ds, x, None, t, zm=start[k])
        zc = cqc.frames_of(ds2, _smoothed(ds2, x2, ft2, sig, **lm))[pos]
        d1, d0 = np.linalg.norm(sr.between(pose[k], zc)), np.linalg.norm(sr.between(start[k], zc))
        print("claim t %.2f: |query - converged| %.3e, |start - converged| %.3e, ratio %.4f" % (t, d1, d0, d1 / d0))
        assert d1 <= 0.5 * d0, (t, d1, d0)


def test_pure_translation_is_exact():
    # both minimisers by the restated LM of tests/smooth_cv_restated.py, as in tests/test_smooth_cv_query_host.py, the query by the device: the
    # claim needs the track converged beyond its bar -- what is left of g goes through H'^-1, and the emptied first frame hangs on pair 0's
    # loose sigmas alone -- and the restated LM runs until no step is accepted
    ds, x0, zt, ft, empty = cqc.translating_sequence()
    sig = (SROT, STRANS, cc.SROT0, cc.STRANS0)
    lm = dict(min_avg=0.0, min_error=0.0, max_iters=100)
    F = len(ft)
    n0 = sc.ns(ds)
    td = tr.TrackData(ds, x0)
    x = np.concatenate([x0[:n0], cv.smooth_lm(cv.SmoothCvProblem(td, *sig, frame_time=ft), td.z0, **lm)["z"].reshape(-1)])
    qt = [ft[0] - 0.7, ft[0] + 0.3, ft[F // 2] - 0.5, ft[-2] + 0.9 * (ft[-1] - ft[-2]), ft[-1] + 2.0]
    with aar.Problem(ds) as p:
        pose = p.track_smooth_query2(x, SROT, STRANS, qt, frame_time=ft, **CV)[0]
        start = p.track_smooth_query2_step(x, SROT, STRANS, qt, frame_time=ft, **CV)[0]
    for k, t in enumerate(qt):
        ds2, x2, ft2, pos = cqc.inserted(ds, x, ft, t, zm=start[k])
        td2 = tr.TrackData(ds2, x2)
        zc = cv.smooth_lm(cv.SmoothCvProblem(td2, *sig, frame_time=ft2), td2.z0, **lm)["z"][pos]
        e = np.abs(pose[k] - zc).max()
        print("translations t %.3f: |query - converged| %.2e" % (t, e))
        assert e <= 1e-9, (t, e)


def test_noiseless_constant_motion_is_returned_at_any_time():
    ds, x0, zt, ft, empty, _ = cc.constant_velocity_sequence()
    sig = (1e-3, 1e-3, 1e3, 1e3)
    x = _smoothed(ds, x0, ft, sig, min_average_step_error_diff=0.0, min_error=0.0, max_iters=100)
    qt = [ft[0] - 0.3, ft[0] - 4.0, ft[0] + 0.4, ft[5] + 0.5 * (ft[6] - ft[5]), ft[6] + 1e-3, ft[-2] + 0.9 * (ft[-1] - ft[-2]), ft[-1] + 0.3,
          ft[-1] + 4.0]
    with aar.Problem(ds) as p:
        pose, cov, _, _ = p.track_smooth_query2(x, sig[0], sig[1], qt, frame_time=ft, model="cv", sigma_rot0=sig[2], sigma_trans0=sig[3])
    w, v = np.array([0.02, -0.025, 0.03]), np.array([0.004, -0.002, 0.003])
    R0 = tr.rodrigues(zt[0][:3])
    for k, t in enumerate(qt):
        truth = np.r_[sr.so3_log(R0 @ tr.rodrigues((t - ft[0]) * w)), zt[0][3:] + (t - ft[0]) * v]
        e = np.abs(pose[k] - truth).max()
        print("constant motion t %.4f: error %.2e" % (t, e))
        assert e < 1e-7, (t, e)
        assert np.linalg.eigvalsh(cov[k])[0] > 0


# ---- 9. the C++ mirror and the command-line driver ----
def _kv(stdout):
    return dict(l.split(" = ") for l in stdout.splitlines() if " = " in l)


def test_mapper_track_smooth_query_overload(tmp_path):
    exe = str(tmp_path / "smooth_cv_query_mapper_main")
    cc_ = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_cv_query_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                          "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr
    ds = aar.synth(2)
    ft = np.asarray(ds.frame_ids, dtype=np.float64)
    qt = np.array([ft[0] - 1.5, ft[0], ft[0] + 0.25, 0.5 * (ft[40] + ft[41]), ft[50], ft[-1] + 2.0])
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS), repr(cc.SROT0), repr(cc.STRANS0)] + [repr(float(t)) for t in qt], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = _kv(run.stdout)
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, _, _, _ = p.track_smooth(xt, SROT, STRANS, frame_time=ft, **CV)
        pose, cov, seg, rep = p.track_smooth_query2(xs, SROT, STRANS, qt, frame_time=ft, **CV)
    assert [int(kv[k]) for k in ("queries", "inside", "on_frame", "outside", "launches")] == \
        [rep[k] for k in ("num_queries", "num_inside", "num_on_frame", "num_outside", "launches")]
    assert (rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (2, 2, 2)
    assert int(kv["same_poses"]) == 1 and int(kv["cov_without"]) == 0 and int(kv["rw_same"]) == 1
    # (the mapper carries its poses as 4x4 matrices between its calls: 1e-8 in the poses as tests/test_gpu_track_smooth.py holds them; the blocks
    # follow the point)
    np.testing.assert_allclose(float(kv["sigma2"]), rep["sigma2"], rtol=1e-7)
    for k in range(len(qt)):
        assert int(kv["segment%d" % k]) == seg[k]
        pm = np.array([float(v) for v in kv["pose%d" % k].split()])
        cm = np.array([float(v) for v in kv["cov%d" % k].split()]).reshape(6, 6)
        assert np.abs(pm - pose[k]).max() <= 1e-8, k
        assert np.abs(cm - cov[k]).max() <= 1e-6 * np.abs(cov[k]).max(), k


def test_find_solution_cv_resample_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # as tests/test_gpu_track_smooth_query.py: the recording is cut before config 2's frames that turn through pi
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    smooth = ["-smooth", repr(SROT), repr(STRANS)]
    cvf = ["-cv", repr(cc.SROT0), repr(cc.STRANS0)]
    run = subprocess.run(base + smooth + cvf + ["-cv-resample", "2"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, AAR_DETERMINISTIC="1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert len([l for l in run.stdout.splitlines() if l.startswith("resample: ")]) == 1 and "smooth: constant velocity" in run.stdout, run.stdout
    sigma2, n, t, seg, pose, blk = parse_resampled_yaml(os.path.join(folder, "final.resampled.yaml"))
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    F = got.num_frames
    ft = np.asarray(got.frame_ids, dtype=np.float64)
    z = got.x_full[n0:n0 + 6 * F].reshape(F, 6)
    assert F == FK and n == 2 and len(t) == 2 * F - 1 and np.linalg.norm(z[:, :3], axis=1).max() < 3.0
    mid = ft[:-1] + (ft[1:] - ft[:-1]) * 0.5
    assert np.array_equal(t[0::2], ft) and np.array_equal(t[1::2], mid)
    assert np.array_equal(seg[0::2], np.arange(F)) and np.array_equal(seg[1::2], np.arange(F - 1))
    with aar.Problem(got) as p:
        pm, cm, _, rep = p.track_smooth_query2(got.x_full, SROT, STRANS, mid, frame_time=ft, **CV)
        S = p.track_smooth_covariance2(got.x_full, SROT, STRANS, frame_time=ft, **CV)[0]
    np.testing.assert_allclose(sigma2, rep["sigma2"], rtol=1e-6)
    assert np.abs(pose[1::2] - pm).max() <= 1e-8 and np.abs(pose[0::2] - z).max() <= 1e-8
    for k in range(F - 1):
        assert np.abs(blk[2 * k + 1] - rep["sigma2"] * cm[k]).max() <= 1e-6 * np.abs(rep["sigma2"] * cm[k]).max(), k
    for f in range(F):
        assert np.abs(blk[2 * f] - rep["sigma2"] * S[f]).max() <= 1e-6 * np.abs(rep["sigma2"] * S[f]).max(), f
    # refused with the usage message: without -cv, without -smooth, together with -live
    os.remove(os.path.join(folder, "final.resampled.yaml"))
    for bad in (base + smooth + ["-cv-resample", "2"], base + cvf + ["-cv-resample", "2"], base + ["-live", "0"] + cvf + ["-cv-resample", "2"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-cv-resample" in run.stdout and "resample: " not in run.stdout, run.stdout
        assert not os.path.exists(os.path.join(folder, "final.resampled.yaml"))
