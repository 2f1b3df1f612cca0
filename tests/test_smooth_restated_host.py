"""The float64 restatement of smoothed tracking (tests/smooth_restated.py) checked on its own, and the host-side validation of
aar_smooth_params.  CPU only."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_restated as sr
import track_restated as tr


# ---- the between factor's complex-step Jacobian against central differences at 60 digits ----
def _mp_rot(w):
    th = mp.sqrt(sum(x * x for x in w))
    W = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + (mp.sin(th) / th) * W + ((1 - mp.cos(th)) / th ** 2) * (W * W)


def _mp_between(x, rel):
    Ra, Rb = _mp_rot(x[0:3]), _mp_rot(x[6:9])
    if rel is not None:
        Ra = Ra * _mp_rot([mp.mpf(float(v)) for v in rel[:3]])
    Q = Ra.T * Rb
    v = [Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]]
    s = mp.sqrt(sum(q * q for q in v)) / 2
    c = (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1) / 2
    th = mp.atan2(s, c)
    k = mp.mpf(1) / 2 if s == 0 else th / (2 * s)
    dt = [0, 0, 0] if rel is None else [mp.mpf(float(q)) for q in rel[3:]]
    return [k * q for q in v] + [x[9 + i] - x[3 + i] - dt[i] for i in range(3)]


def _mp_jacobian(za, zb, rel):
    mp.mp.dps = 60
    x0 = [mp.mpf(float(v)) for v in np.concatenate([za, zb])]
    h = mp.mpf(10) ** -20
    J = np.zeros((6, 12))
    for k in range(12):
        xp, xm = list(x0), list(x0)
        xp[k] += h
        xm[k] -= h
        ep, em = _mp_between(xp, rel), _mp_between(xm, rel)
        J[:, k] = [float((a - b) / (2 * h)) for a, b in zip(ep, em)]
    return J, np.array([float(v) for v in _mp_between(x0, rel)])


def _pairs():
    rng = np.random.default_rng(5)
    out = []
    for i in range(6):                                    # generic pairs (the relative rotation kept below 3 rad)
        za = rng.normal(size=6) * [0.8, 0.8, 0.8, 1, 1, 1]
        zb = za + rng.normal(size=6) * 0.4
        out.append((za, zb, rng.normal(size=6) * 0.2 if i % 2 else None))
    za = rng.normal(size=6)
    for eps in (0.0, 1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 2e-3):   # theta -> 0, both sides of the series switch (sin^2 = 1e-6)
        zb = np.array(za)
        zb[:3] = sr.so3_log(tr.rodrigues(za[:3]) @ tr.rodrigues(np.array([0.6, -0.64, 0.48]) * eps))
        zb[3:] += 0.1
        out.append((za, zb, None))
    for th in (2.5, 2.9, 2.99):                           # theta ~ 3
        zb = np.array(za)
        zb[:3] = sr.so3_log(tr.rodrigues(za[:3]) @ tr.rodrigues(np.array([0.0, 0.6, 0.8]) * th))
        out.append((za, zb, None))
    return out


@pytest.mark.parametrize("i", range(16))
def test_between_jacobian_against_central_differences(i):
    za, zb, rel = _pairs()[i]
    J, e = sr.between_jacobian(za, zb, rel)
    Jr, er = _mp_jacobian(za, zb, rel)
    # ~100 float64 operations on entries of order 1 behind each derivative, amplified by 1 / sin(theta) <= 7 at theta = 2.99 and by the
    # rotation-vector chart's own Jacobian (<= ~3 here): 1e-11 is two orders above that and nine below the entries
    assert np.abs(e - er).max() < 1e-13
    assert np.abs(J - Jr).max() < 1e-11, np.abs(J - Jr).max()


# ---- Lambda -> 0: the joint minimiser is track()'s, frame by frame ----
def test_vanishing_prior_gives_the_per_frame_minimiser():
    ds = aar.synth(2, num_frames=12)
    x0 = sc.track_start(ds)
    xt, res = tr.track_all(ds, x0, min_avg=0.0)
    td = tr.TrackData(ds, x0)
    r = sr.smooth_lm(sr.SmoothProblem(td, 1e12, 1e12), td.z0, min_avg=0.0)
    zt = xt[sc.ns(ds):].reshape(-1, 6)
    assert np.abs(r["z"] - zt).max() < 1e-7, np.abs(r["z"] - zt).max()
    assert r["prior"] < 1e-20


# ---- the linear algebra of the restatement: banded and dense agree, and against a long double solve ----
def test_banded_solve_against_long_double():
    ds = aar.synth(2, num_frames=9)
    td = tr.TrackData(ds, sc.track_start(ds))
    sp = sr.SmoothProblem(td, 0.05, 0.02, frame_time=np.array([0, 1, 2, 7, 8, 9, 10, 11, 12.0]))
    diag, off, rhs = sp.system(td.z0)
    H = sr.dense(diag, off)
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    mu = 1e-3 * np.max(np.einsum("fii->fi", diag))
    d = sr.solve(diag, off, rhs, mu)
    # iterative refinement with long double residuals: the solution to ~1e-19 relative
    A = (H + mu * np.eye(len(rhs))).astype(np.longdouble)
    x = d.astype(np.longdouble)
    for _ in range(5):
        x = x + np.linalg.solve(H + mu * np.eye(len(rhs)), (rhs.astype(np.longdouble) - A @ x).astype(np.float64)).astype(np.longdouble)
    assert float(np.abs(d - x).max() / np.abs(x).max()) < 1e-9
    assert np.abs(sr.matvec(diag, off, d, mu) - rhs).max() <= 1e-10 * np.abs(rhs).max()


# ---- aar_smooth_params_validate ----
def _invalid(*a, **k):
    with pytest.raises(aar.AarError) as e:
        aar.smooth_params_validate(*a, **k)
    assert e.value.code == aar.AAR_ERR_INVALID
    return str(e.value)


def test_validate_accepts_null_arrays_and_good_ones():
    aar.smooth_params_validate(10, 0.01, 0.02)
    aar.smooth_params_validate(0, 0.01, 0.02)
    aar.smooth_params_validate(1, 0.01, 0.02, frame_time=[3.0], rel_motion=np.zeros((0, 6)))
    aar.smooth_params_validate(4, 0.01, 0.02, frame_time=[0, 1, 5, 6.5], rel_motion=np.zeros((3, 6)))
    # a struct that ends after the sigmas: the arrays read as NULL
    aar.smooth_params_validate(4, 0.01, 0.02, struct_size=aar.CSmoothParams.frame_time.offset)


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_validate_rejects_bad_sigmas(bad):
    assert "sigma_rot" in _invalid(5, bad, 0.02)
    assert "sigma_trans" in _invalid(5, 0.01, bad)


def test_validate_names_the_offending_index():
    assert "frame_time[2]" in _invalid(4, 0.01, 0.02, frame_time=[0, 1, 1, 2])
    assert "frame_time[3]" in _invalid(4, 0.01, 0.02, frame_time=[0, 1, 2, 1.5])
    assert "frame_time[1]" in _invalid(4, 0.01, 0.02, frame_time=[0, float("nan"), 2, 3])
    rel = np.zeros((3, 6))
    rel[2, 4] = float("inf")
    assert "rel_motion[2][4]" in _invalid(4, 0.01, 0.02, rel_motion=rel)
    rel[2, 4] = 0.0
    rel[0, 0] = float("nan")
    assert "rel_motion[0][0]" in _invalid(4, 0.01, 0.02, rel_motion=rel)


def test_validate_rejects_a_struct_without_the_sigmas():
    assert "struct_size" in _invalid(4, 0.01, 0.02, struct_size=aar.CSmoothParams.sigma_trans.offset)
    assert "struct_size" in _invalid(4, 0.01, 0.02, struct_size=4)
    with pytest.raises(aar.AarError):
        aar._check(aar.lib().aar_smooth_params_validate(3, None))
    assert C.sizeof(aar.CSmoothParams) == 40 and C.sizeof(aar.CSmoothReport) == 64


# ---- noise reduction where it must occur, on the restatement alone ----
def test_static_object_is_pooled():
    # 64 frames of one pose with independent corner noise, sigma = 1e-5: the prior all but equates the 64 poses, so their common error
    # is that of 64 pooled frames, 1 / sqrt(64) = 1/8 of one frame's.  Measured with this seed: ratio 0.123.
    ds, x0, zt = sc.static_object()
    xt, _ = tr.track_all(ds, x0)
    td = tr.TrackData(ds, xt)
    r = sr.smooth_lm(sr.SmoothProblem(td, 1e-5, 1e-5), td.z0)
    xs = np.array(xt)
    xs[sc.ns(ds):] = r["z"].reshape(-1)
    a, b = sc.pose_rms(xs, ds, zt), sc.pose_rms(xt, ds, zt)
    print("static object: rms smooth %.3e, track %.3e, ratio %.3f" % (a, b, a / b))
    assert a <= 0.5 * b, (a, b)
