"""The restatement of aar_track_smooth_relative (tests/smooth_relative_restated.py) checked on its own -- the Gauss-Markov
chain on frames and on supernodes against numpy.linalg.inv of the dense H of the existing restatements, the closed-form rel_cov against
J Sigma J^T with the complex-step Jacobian -- and the refusals of aar_smooth_relative_validate.  CPU only.
"""
import ctypes as C

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_cv_restated as cv
import smooth_relative_cases as rc
import smooth_relative_restated as rr
import smooth_restated as sr
import track_restated as tr

EPS = np.finfo(np.float64).eps
SROT, STRANS = rc.SROT, rc.STRANS


def _restated(model, F):
    """(H dense, z [F, 6]) of the restated system at the start poses: emptied frames from four frames on, uneven frame times"""
    ds = rc.dataset(F)
    td = tr.TrackData(ds, sc.track_start(ds))
    ft = rc.times(F)
    if model == "cv":
        sp = cv.SmoothCvProblem(td, SROT, STRANS, cc.SROT0, cc.STRANS0, frame_time=ft)
        diag, off, off2, _ = sp.system(td.z0)
        return cv.dense(diag, off, off2), np.array(td.z0)
    sp = sr.SmoothProblem(td, SROT, STRANS, frame_time=ft)
    diag, off, _ = sp.system(td.z0)
    return sr.dense(diag, off), np.array(td.z0)


def _cross(model, Sigma, F):
    """the restated chain's answer to every pair: [F, F, 6, 6]"""
    if model == "cv":
        S12, R12 = rr.cv_blocks(Sigma, F)
        return np.array([[rr.cv_cross(S12, R12, a, b) for b in range(F)] for a in range(F)])
    S, R = rr.rw_blocks(Sigma, F)
    return np.array([[rr.rw_cross(S, R, a, b) for b in range(F)] for a in range(F)])


@pytest.mark.parametrize("F", rc.SIZES)
@pytest.mark.parametrize("model", ["rw", "cv"])
def test_chain_against_the_inverse(model, F):
    H, _ = _restated(model, F)
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    kappa = float(ev[-1] / ev[0])
    Sigma = np.linalg.inv(H)
    got = _cross(model, Sigma, F)
    want = Sigma.reshape(F, 6, F, 6).transpose(0, 2, 1, 3)
    big = float(np.abs(Sigma).max())
    lag = np.abs(np.arange(F)[:, None] - np.arange(F)[None, :])
    by_lag = [float(np.abs(got - want)[lag == l].max() / big) for l in range(F)]
    print("%s F %d: kappa %.3e, error by lag in eps kappa: %s" % (model, F, kappa, " ".join("%.4f" % (e / (EPS * kappa)) for e in by_lag)))
    assert max(by_lag) <= 10 * EPS * kappa, (by_lag, 10 * EPS * kappa)
    # what exists is taken, not chained: the lags the selected inverse holds are Sigma's own bits
    upper = np.arange(F)[:, None] <= np.arange(F)[None, :]          # (numpy's inverse is not symmetric to the bit: the blocks with a <= b)
    # (under constant velocity lag three from an odd frame spans three supernodes: a chain of one step, as in aar_track_smooth_lag3)
    node = np.arange(F) // 2 if model == "cv" else np.arange(F)
    held = (np.abs(node[:, None] - node[None, :]) <= 1) & upper
    assert lag[held].max() == min(rr.direct_lag(model), F - 1)
    assert np.array_equal(got[held], want[held])
    # (b, a) is the transpose of (a, b) to the bit (a = b is Sigma's own diagonal block)
    off = lag > 0
    assert np.array_equal(got[off], got.transpose(1, 0, 3, 2)[off])


def test_supernode_blocks_of_an_odd_track():
    F = 5
    rng = np.random.default_rng(1)
    A = rng.normal(size=(6 * F, 6 * F))
    Sigma = A @ A.T
    S12, R12 = rr.cv_blocks(Sigma, F)
    assert S12.shape == (3, 12, 12) and R12.shape == (2, 12, 12)
    assert np.array_equal(S12[2][:6, :6], rr.block(Sigma, 4, 4)) and np.array_equal(S12[2][6:, 6:], np.eye(6)) and not S12[2][:6, 6:].any()
    assert np.array_equal(R12[1][:6, :6], rr.block(Sigma, 2, 4)) and np.array_equal(R12[1][6:, :6], rr.block(Sigma, 3, 4)) and not R12[1][:, 6:].any()
    assert np.array_equal(R12[0][:6, 6:], rr.block(Sigma, 0, 3))


def _poses():
    rng = np.random.default_rng(11)
    out = []
    for scale in (0.0, 1e-9, 1e-5, 1e-3, 0.3, 1.0, 2.0):          # the relative rotation from zero to large, both sides of the series switches
        za = rng.normal(size=6) * [0.8, 0.8, 0.8, 1, 1, 1]
        zb = np.array(za)
        zb[:3] = sr.so3_log(tr.rodrigues(za[:3]) @ tr.rodrigues(np.array([0.6, -0.64, 0.48]) * scale))
        zb[3:] += rng.normal(size=3) * 0.2
        out.append((za, zb))
    return out


@pytest.mark.parametrize("i", range(7))
def test_rel_cov_against_the_complex_step(i):
    za, zb = _poses()[i]
    rng = np.random.default_rng(5 + i)
    # a joint covariance of two strongly correlated frames: a shared error plus a small one of each frame's own
    A, B = rng.normal(size=(6, 6)), rng.normal(size=(12, 12)) * 0.05
    Sj = np.kron(np.ones((2, 2)), A @ A.T) + B @ B.T
    Saa, Sab, Sbb = Sj[:6, :6], Sj[:6, 6:], Sj[6:, 6:]
    got = rr.rel_cov(za, zb, Saa, Sbb, Sab)
    want = rr.rel_cov_complex_step(za, zb, Saa, Sbb, Sab)
    big = max(float(np.abs(t).max()) for t in rr.summands(za, zb, Saa, Sbb, Sab))
    err = float(np.abs(got - want).max())
    print("pair %d: |phi| %.3e, largest summand %.3e, rel_cov %.3e, error %.3e" % (i, np.linalg.norm(rr.rel(za, zb)[:3]), big, np.abs(want).max(), err))
    # the closed-form Jacobians and the complex-step ones agree to the 1e-11 that tests/test_smooth_restated_host.py holds the latter to against
    # 60-digit differences; rel_cov is bilinear in them
    assert err <= 4e-11 * big, (err, big)
    assert np.array_equal(got, got.T) or np.abs(got - got.T).max() <= 8 * EPS * big
    Ja, Jb = rr.jacobians(za, zb)
    J, e = sr.between_jacobian(za, zb)
    assert np.abs(np.hstack([Ja, Jb]) - J).max() <= 1e-11
    assert np.array_equal(rr.rel(za, zb), e)
    # the same pose twice: no motion
    assert not rr.rel(za, za).any()


def test_counts():
    pairs = [(0, 0), (0, 1), (3, 1), (1, 4), (9, 2)]
    assert rr.counts(pairs, "rw") == (2, 3, 7) and rr.counts(pairs, "cv") == (4, 1, 7) and rr.counts(np.zeros((0, 2)), "cv") == (0, 0, 0)


# ---- aar_smooth_relative_validate ----
def _refused(what, *args, **kw):
    with pytest.raises(aar.AarError) as e:
        aar.smooth_relative_validate(*args, **kw)
    assert e.value.code == aar.AAR_ERR_INVALID and what in str(e.value), str(e.value)


@pytest.mark.parametrize("model", ["rw", "cv"])
def test_validate(model):
    kw = rc.MODELS[model]
    aar.smooth_relative_validate(5, SROT, STRANS, [(0, 4), (4, 0), (2, 2), (0, 4)], **kw)
    aar.smooth_relative_validate(5, SROT, STRANS, np.zeros((0, 2)), **kw)
    aar.smooth_relative_validate(0, SROT, STRANS, np.zeros((0, 2)), **kw)
    aar.smooth_relative_validate(5, SROT, STRANS, [(0, 4)])                       # the struct without the model fields
    _refused("frame_a[1] = 5", 5, SROT, STRANS, [(0, 4), (5, 0)], **kw)
    _refused("frame_a[2] = -1", 5, SROT, STRANS, [(0, 4), (1, 1), (-1, 0)], **kw)
    _refused("frame_b[0] = 5", 5, SROT, STRANS, [(0, 5)], **kw)
    _refused("frame_b[3] = -7", 5, SROT, STRANS, [(0, 0), (1, 1), (2, 2), (3, -7)], **kw)
    _refused("frame_a[0] = 0", 0, SROT, STRANS, [(0, 0)], **kw)                    # no frame at all
    _refused("sigma_rot", 5, -1.0, STRANS, [(0, 1)], **kw)                         # whatever aar_smooth_params_validate refuses
    _refused("frame_time[2]", 5, SROT, STRANS, [(0, 1)], frame_time=[0.0, 1.0, 1.0, 2.0, 3.0], **kw)
    if model == "cv":
        _refused("sigma_rot0", 5, SROT, STRANS, [(0, 1)], model="cv", sigma_rot0=0.0, sigma_trans0=1.0)


def test_validate_null_arrays_and_counts():
    sp = aar.SmoothParams(SROT, STRANS)
    ip = C.POINTER(C.c_int32)
    one = np.zeros(1, dtype=np.int32)
    L = aar.lib()
    assert L.aar_smooth_relative_validate(3, C.byref(sp.c), 0, None, None) == 0
    assert L.aar_smooth_relative_validate(3, C.byref(sp.c), 1, None, one.ctypes.data_as(ip)) == aar.AAR_ERR_INVALID
    assert "frame_a is NULL" in aar.lib().aar_last_error().decode()
    assert L.aar_smooth_relative_validate(3, C.byref(sp.c), 1, one.ctypes.data_as(ip), None) == aar.AAR_ERR_INVALID
    assert "frame_b is NULL" in aar.lib().aar_last_error().decode()
    assert L.aar_smooth_relative_validate(3, C.byref(sp.c), -1, one.ctypes.data_as(ip), one.ctypes.data_as(ip)) == aar.AAR_ERR_INVALID
    assert "n_pairs = -1" in aar.lib().aar_last_error().decode()
    assert L.aar_smooth_relative_validate(3, None, 0, None, None) == aar.AAR_ERR_INVALID
