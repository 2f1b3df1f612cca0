"""The constant-velocity smoother's restatement (tests/smooth_cv_restated.py) checked on its own, the parameter checks
of include/aar.h, and the claim of the model: a frame without detections at either end of the sequence is extrapolated, not held.  CPU only.
"""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_cv_restated as cv
import smooth_restated as sr
import track_restated as tr


# ---- the 6x18 Jacobian against 60-digit central differences ----
def _mp_rot(w):
    W = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    th = mp.sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + (mp.sin(th) / th) * W + ((1 - mp.cos(th)) / th ** 2) * (W * W)


def _mp_log(Q):
    v = [Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]]
    s = mp.sqrt(sum(q * q for q in v)) / 2
    c = (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1) / 2
    th = mp.atan2(s, c)
    k = mp.mpf(1) / 2 if s == 0 else th / (2 * s)
    return [k * q for q in v]


def _mp_term(x, r):
    Rp, Rc, Rn = _mp_rot(x[0:3]), _mp_rot(x[6:9]), _mp_rot(x[12:15])
    psi = _mp_log(Rp.T * Rc)
    dR = _mp_rot([r * q for q in psi])
    phi = _mp_log((Rc * dR).T * Rn)
    return phi + [x[15 + i] - x[9 + i] - r * (x[9 + i] - x[3 + i]) for i in range(3)]


def _mp_jacobian(zp, zc, zn, r):
    mp.mp.dps = 60
    x0 = [mp.mpf(float(v)) for v in np.concatenate([zp, zc, zn])]
    r = mp.mpf(float(r))
    h = mp.mpf(10) ** -20
    J = np.zeros((6, 18))
    for k in range(18):
        xp, xm = list(x0), list(x0)
        xp[k] += h
        xm[k] -= h
        ep, em = _mp_term(xp, r), _mp_term(xm, r)
        J[:, k] = [float((a - b) / (2 * h)) for a, b in zip(ep, em)]
    return J, np.array([float(v) for v in _mp_term(x0, r)])


def _triples():
    rng = np.random.default_rng(7)
    out = []
    for i in range(6):                                    # generic triples, every ratio twice
        zp = rng.normal(size=6) * [0.8, 0.8, 0.8, 1, 1, 1]
        zc = zp + rng.normal(size=6) * 0.3
        zn = zc + rng.normal(size=6) * 0.3
        out.append((zp, zc, zn, (0.5, 1.0, 3.0)[i % 3]))
    zp = rng.normal(size=6)
    for i, eps in enumerate((0.0, 1e-12, 1e-9, 1e-6, 1e-4, 1e-3, 2e-3)):   # psi -> 0, both sides of the series switches
        zc = np.array(zp)
        zc[:3] = sr.so3_log(tr.rodrigues(zp[:3]) @ tr.rodrigues(np.array([0.6, -0.64, 0.48]) * eps))
        zc[3:] += 0.1
        zn = zc + rng.normal(size=6) * 0.2
        out.append((zp, zc, zn, (0.5, 1.0, 3.0)[i % 3]))
    zc = zp + rng.normal(size=6) * 0.2
    for i, th in enumerate((2.5, 2.9, 2.99)):             # |phi| ~ 3
        r = (0.5, 1.0, 3.0)[i]
        dR = tr.rodrigues(r * sr.so3_log(tr.rodrigues(zp[:3]).T @ tr.rodrigues(zc[:3])))
        zn = np.array(zc)
        zn[:3] = sr.so3_log(tr.rodrigues(zc[:3]) @ dR @ tr.rodrigues(np.array([0.0, 0.6, 0.8]) * th))
        out.append((zp, zc, zn, r))
    return out


@pytest.mark.parametrize("i", range(16))
def test_term_jacobian_against_central_differences(i):
    zp, zc, zn, r = _triples()[i]
    J, e = cv.cv_term_jacobian(zp, zc, zn, r)
    Jr, er = _mp_jacobian(zp, zc, zn, r)
    if i >= 13:
        assert 2.4 < np.linalg.norm(e[:3]) < 3.0
    # the bar and the argument of tests/test_smooth_restated_host.py: ~100 float64 operations on entries of order 1 behind each derivative,
    # amplified by 1 / sin(theta) <= 7 at theta = 2.99 and by the charts' own Jacobians (here also r <= 3 through dR): 1e-11 is two orders
    # above that and nine below the entries
    assert np.abs(e - er).max() < 1e-13
    assert np.abs(J - Jr).max() < 1e-11, np.abs(J - Jr).max()


def test_translation_rows_are_constant():
    zp, zc, zn, r = _triples()[2]
    J, _ = cv.cv_term_jacobian(zp, zc, zn, r)
    want = np.zeros((3, 18))
    for k, c in enumerate((r, -(1 + r), 1.0)):
        want[:, 6 * k + 3: 6 * k + 6] = c * np.eye(3)
    assert np.abs(J[3:] - want).max() < 1e-15


# ---- the linear algebra of the restatement ----
def _small(F=9, **kw):
    ds = aar.synth(2, num_frames=F)
    td = tr.TrackData(ds, sc.track_start(ds))
    return td, cv.SmoothCvProblem(td, cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0, **kw)


def test_banded_solve_against_the_dense_solve():
    td, sp = _small(frame_time=np.array([0, 1, 2, 7, 8, 9, 10, 11, 12.0]))
    diag, off, off2, rhs = sp.system(td.z0)
    H = cv.dense(diag, off, off2)
    assert np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    assert np.linalg.eigvalsh(H).min() > 0                 # positive definite at mu = 0
    assert np.abs(off2).max() > 0
    for mu in (0.0, 1e-3 * np.max(np.einsum("fii->fi", diag))):
        d = cv.solve(diag, off, off2, rhs, mu)
        dd = cv.solve(diag, off, off2, rhs, mu, use_banded=False)
        assert np.abs(d - dd).max() <= 1e-9 * np.abs(dd).max()
        assert np.abs(cv.matvec(diag, off, off2, d, mu) - rhs).max() <= 1e-10 * np.abs(rhs).max()
        assert np.abs((H + mu * np.eye(len(rhs))) @ d - cv.matvec(diag, off, off2, d, mu)).max() <= 1e-12 * np.abs(rhs).max()


def test_system_is_the_gradient_of_the_cost():
    td, sp = _small(F=6)
    z = td.z0
    _, _, _, rhs = sp.system(z)
    g = np.zeros(z.size)
    for k in range(z.size):
        d = np.zeros(z.size)
        d[k] = 1e-6
        g[k] = (sp.cost(z + d.reshape(z.shape)) - sp.cost(z - d.reshape(z.shape))) / 2e-6
    assert np.abs(-0.5 * g - rhs).max() <= 1e-6 * np.abs(rhs).max()      # b = -J^T r = -grad E / 2


def test_sizes_without_a_term():
    for F in (1, 2):
        td, sp = _small(F=F)
        diag, off, off2, rhs = sp.system(td.z0)
        assert diag.shape == (F, 6, 6) and off.shape == (F - 1, 6, 6) and off2.shape == (0, 6, 6)
        assert len(sp.costs(td.z0)[1]) == F - 1 and sp.rows == 8.0 * (td.start[F] - td.start[0]) + 6.0 * (F - 1)
    # F = 2 is the random walk with pair 0's sigmas
    rw = sr.SmoothProblem(td, cc.SROT0, cc.STRANS0)
    for a, b in zip(rw.system(td.z0), (diag, off, rhs)):
        assert np.array_equal(a, b)


# ---- sigma -> infinity: the joint minimiser is track()'s, frame by frame ----
def test_vanishing_prior_gives_the_per_frame_minimiser():
    ds = aar.synth(2, num_frames=12)
    x0 = sc.track_start(ds)
    xt, _ = tr.track_all(ds, x0, min_avg=0.0)
    td = tr.TrackData(ds, x0)
    r = cv.smooth_lm(cv.SmoothCvProblem(td, 1e12, 1e12, 1e12, 1e12), td.z0, min_avg=0.0)
    zt = xt[sc.ns(ds):].reshape(-1, 6)
    assert np.abs(r["z"] - zt).max() < 1e-7, np.abs(r["z"] - zt).max()
    assert r["prior"] < 1e-20


# ---- aar_smooth_params_validate ----
CV = dict(model="cv", sigma_rot0=1.0, sigma_trans0=1.0)


def _invalid(*a, **k):
    with pytest.raises(aar.AarError) as e:
        aar.smooth_params_validate(*a, **k)
    assert e.value.code == aar.AAR_ERR_INVALID
    return str(e.value)


def test_validate_accepts():
    aar.smooth_params_validate(10, 0.01, 0.02, **CV)
    aar.smooth_params_validate(0, 0.01, 0.02, **CV)
    aar.smooth_params_validate(4, 0.01, 0.02, frame_time=[0, 1, 5, 6.5], **CV)
    aar.smooth_params_validate(4, 0.01, 0.02, frame_time=[0, 1, 5, 6.5], rel_motion=np.zeros((3, 6)), model="rw")
    aar.smooth_params_validate(4, 0.01, 0.02, model="rw", sigma_rot0=-1.0, sigma_trans0=float("nan"))   # unused under the random walk


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")])
def test_validate_rejects_bad_sigmas_by_field(bad):
    assert "sigma_rot0" in _invalid(5, 0.01, 0.02, model="cv", sigma_rot0=bad, sigma_trans0=1.0)
    assert "sigma_trans0" in _invalid(5, 0.01, 0.02, model="cv", sigma_rot0=1.0, sigma_trans0=bad)
    assert "sigma_rot " in _invalid(5, bad, 0.02, **CV)
    assert "sigma_trans " in _invalid(5, 0.01, bad, **CV)


def test_validate_rejects_rel_motion_and_unknown_models():
    assert "rel_motion" in _invalid(4, 0.01, 0.02, rel_motion=np.zeros((3, 6)), **CV)
    assert "model" in _invalid(4, 0.01, 0.02, model=2, sigma_rot0=1.0, sigma_trans0=1.0)
    assert "model" in _invalid(4, 0.01, 0.02, model=-1)
    assert "frame_time[2]" in _invalid(4, 0.01, 0.02, frame_time=[0, 1, 1, 2], **CV)


def test_struct_size_versioning():
    assert C.sizeof(aar.CSmoothParams) == 40 and C.sizeof(aar.CSmoothParamsV2) == 64
    assert aar.CSmoothParamsV2.model.offset == 40 and aar.CSmoothParamsV2.sigma_rot0.offset == 48 and aar.CSmoothParamsV2.sigma_trans0.offset == 56
    # a 40-byte struct is the random walk whatever memory follows it: a model the library would refuse, sigmas it would refuse, rel_motion set
    rel = np.zeros((3, 6))
    aar.smooth_params_validate(4, 0.01, 0.02, rel_motion=rel, struct_size=40, model=7, sigma_rot0=-1.0, sigma_trans0=float("nan"))
    aar.smooth_params_validate(4, 0.01, 0.02, rel_motion=rel, struct_size=40, **CV)
    # ... and one that ends inside the model field too (a field counts only when the struct holds it whole)
    aar.smooth_params_validate(4, 0.01, 0.02, rel_motion=rel, struct_size=42, **CV)
    # the model without its sigmas: they read as 0 and are refused by name
    assert "sigma_rot0" in _invalid(4, 0.01, 0.02, struct_size=44, **CV)
    assert "sigma_trans0" in _invalid(4, 0.01, 0.02, struct_size=56, **CV)
    aar.smooth_params_validate(4, 0.01, 0.02, struct_size=64, **CV)
    assert "aar_track_smooth_system2" in aar.SYMBOLS and hasattr(C.CDLL(aar.LIB_PATH), "aar_track_smooth_system2")


# ---- the claim: the emptied end frames are extrapolated ----
def test_emptied_end_frames_are_extrapolated():
    # measured here: err_cv / err_rw = 0.061 at frame 0 and 0.086 at frame 99; both below 0.25, so the bar is 0.5.
    # LM: the average-step stop off and 14 iterations -- a frame without detections moves on the prior's cost alone, which that stop
    # cuts short (at the default stop the ratios are 0.15 and 0.28); after 14 iterations the end frames have moved to within 1e-7 of the
    # minimiser's and every decision of the run is still decided (margin 3e-6), so the device can be held to the same run.
    ds, x0, empty = cc.claim_case()
    assert ds.num_frames == 100 and empty[0] == 0 and empty[-1] == 99 and len(empty) == 12
    td = tr.TrackData(ds, x0)
    r_cv = cv.smooth_lm(cv.SmoothCvProblem(td, cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0), td.z0, **cc.TIGHT)
    r_rw = sr.smooth_lm(sr.SmoothProblem(td, cc.SROT, cc.STRANS), td.z0, **cc.TIGHT)
    e_cv, e_rw = cc.end_errors(r_cv["z"], ds), cc.end_errors(r_rw["z"], ds)
    print("end frames: cv %.3e %.3e, rw %.3e %.3e, ratio %.3f %.3f; margins %.1e %.1e"
          % (e_cv + e_rw + (e_cv[0] / e_rw[0], e_cv[1] / e_rw[1], r_cv["margin"], r_rw["margin"])))
    assert r_cv["margin"] > 1e-9
    assert e_cv[0] <= 0.5 * e_rw[0] and e_cv[1] <= 0.5 * e_rw[1], (e_cv, e_rw)


# ---- exactness on an object in constant motion ----
def test_constant_motion_is_reproduced_exactly():
    ds, x0, zt, ft, empty, wn = cc.constant_velocity_sequence()
    assert np.ptp(np.diff(ft)) > 0 and np.all(np.bincount(ds.obs_frame, minlength=len(ft))[empty] == 0)
    td = tr.TrackData(ds, x0)
    lm = dict(min_avg=0.0, min_error=0.0, max_iters=100)
    # sigma_*0 = 1e3: pair 0 is a random-walk term and is not zero at the truth; loose enough, it does not hold the emptied first frame back.
    # sigma = 1e-3: any value reproduces the truth, a tight one averages the float32 rounding of the corners over all frames
    sp = cv.SmoothCvProblem(td, 1e-3, 1e-3, 1e3, 1e3, frame_time=ft)
    Pe = sp.costs(zt)[1]
    assert Pe[1:].sum() <= 1e-20, Pe[1:].sum()             # every constant-velocity term vanishes at the truth
    r = cv.smooth_lm(sp, td.z0, **lm)
    err = np.abs(r["z"] - zt).max(axis=1)
    print("constant motion: max error %.2e (emptied frames %s)" % (err.max(), err[empty]))
    assert err.max() < 1e-7, err
    # the random walk holds the emptied end frames at their neighbours: off by a step of the motion
    rw = sr.smooth_lm(sr.SmoothProblem(td, cc.SROT, cc.STRANS, frame_time=ft), td.z0, **lm)
    for f, step in ((0, ft[1] - ft[0]), (len(ft) - 1, ft[-1] - ft[-2])):
        miss = np.linalg.norm(rw["z"][f, :3] - zt[f, :3])
        assert 0.5 * wn * step < miss < 1.5 * wn * step, (f, miss, wn * step)
