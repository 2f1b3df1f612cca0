"""The numpy restatement of a smoothed track's pose covariance at any time (tests/smooth_query_restated.py) against numpy.linalg.inv of the dense
AUGMENTED system -- the frame inserted at the query's time and geodesic pose, without detections -- on systems of tests/smooth_restated.py, and the
interface of aar_track_smooth_query as header and binding declare it.  CPU only.

Bar: Frobenius error of the queried block over the Frobenius norm of the yardstick's block <= 10 eps kappa_2(H'), H' the augmented matrix:
the forward-error order of any inverse, not a measured figure.  The restatement takes S and R from numpy's inverse of the
original H and does the kernel's 6x6 block algebra, so the cancellation in P^-1 - F is part of what is measured."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_covariance_restated as scr
import smooth_query_cases as sqc
import smooth_query_restated as sqr
import smooth_restated as sr
import track_restated as tr
from conftest import ROOT
from test_smooth_covariance_host import _base, _resized

EPS = np.finfo(np.float64).eps
SROT, STRANS = 0.05, 0.02
ALPHAS = [1e-3, 0.1, 0.5, 0.9]
EMPTY = {1: [], 2: [], 3: [1], 12: [4, 5, 8]}


def _times(F, uniform):
    return None if uniform else np.cumsum(np.r_[0.5, 1.0 + (np.arange(F - 1) % 3 == 1) * 2.5 + 0.25 * (np.arange(F - 1) % 2)])


def _turned(ds, step):
    """the data set with the frames' rotation vectors moved apart: inter-frame rotations of up to about `step` rad"""
    F = ds.num_frames
    n0 = sc.ns(ds)
    x = np.array(ds.x_full)
    z = x[n0:n0 + 6 * F].reshape(F, 6)
    rng = np.random.default_rng(11)
    u = rng.normal(size=(F, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    z[:, :3] += np.cumsum(u * step * np.linspace(0.0, 1.0, F)[:, None], axis=0)
    return sc.copy_of(ds, x_full=x)


def _problem(F, uniform, empty, step=0.3):
    ds = sc.without_frames(_turned(_resized(_base("g_track_cfg2"), F), step), empty)
    return ds, np.array(ds.x_full), _times(F, uniform)


def _dense_system(ds, x, ft):
    td = tr.TrackData(ds, x)
    diag, off, _ = sr.SmoothProblem(td, SROT, STRANS, frame_time=ft).system(td.z0)
    return sr.dense(diag, off)


def _queries(F, times):
    """(tag, t) of the cases: every alpha in the first and the last gap and in the gaps beside / between emptied frames, both extrapolations"""
    out = []
    gaps = sorted({0, F - 2} | {g for e in EMPTY[F] for g in (e - 1, e)}) if F > 1 else []
    for g in gaps:
        for al in ALPHAS:
            out.append(("gap %d alpha %g" % (g, al), times[g] + al * (times[g + 1] - times[g])))
    for d in (0.3, 4.0):
        out.append(("before %g" % d, times[0] - d))
        out.append(("after %g" % d, times[-1] + d))
    return out


WORST = {}


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("F", [1, 2, 3, 12])
def test_restated_query_against_the_dense_augmented_inverse(F, uniform):
    ds, x, ft = _problem(F, uniform, EMPTY[F])
    times = sqr.times_of(F, ft)
    z = sqc.frames_of(ds, x)
    if F > 1:
        turn = max(np.linalg.norm(sr.between(z[f], z[f + 1])[:3]) for f in range(F - 1))
        assert turn < 0.35 and (F < 12 or turn > 0.2), turn
    S, R = scr.selected_blocks(np.linalg.inv(_dense_system(ds, x, ft)), F)
    worst = 0.0
    for tag, t in _queries(F, times):
        ds2, x2, ft2, pos = sqc.inserted(ds, x, ft, t)
        H2 = _dense_system(ds2, x2, ft2)
        kappa = np.linalg.cond(H2)
        want = np.linalg.inv(H2)[6 * pos:6 * pos + 6, 6 * pos:6 * pos + 6]
        got = sqr.block_form(z, times, S, R, t, SROT, STRANS)
        plain = sqr.plain_form(z, times, S, R, t, SROT, STRANS)
        e_b = np.linalg.norm(got - want) / np.linalg.norm(want)
        e_p = np.linalg.norm(plain - want) / np.linalg.norm(want)
        print("F %d %s %s: kappa %.2e, block form %.2e = %.4f eps kappa, plain form %.2e" %
              (F, "uniform" if uniform else "gaps", tag, kappa, e_b, e_b / (EPS * kappa), e_p))
        assert e_b <= 10 * EPS * kappa and e_p <= 10 * EPS * kappa, (tag, e_b, e_p, EPS * kappa)
        worst = max(worst, e_b / (EPS * kappa))
        np.testing.assert_allclose(sqc.frames_of(ds2, x2)[pos], sqr.pose(z, times, t), rtol=0, atol=0)
    WORST[(F, uniform)] = worst
    print("F %d: the largest block-form error is %.4f eps kappa_2(H')" % (F, worst))


def test_on_a_frame_time_and_locate():
    ds, x, ft = _problem(12, False, EMPTY[12])
    times = sqr.times_of(12, ft)
    z = sqc.frames_of(ds, x)
    S, R = scr.selected_blocks(np.linalg.inv(_dense_system(ds, x, ft)), 12)
    for f in (0, 5, 11):
        assert sqr.locate(times, times[f]) == (f, "on")
        assert np.array_equal(sqr.pose(z, times, times[f]), z[f])
        assert np.array_equal(sqr.block_form(z, times, S, R, times[f], SROT, STRANS), S[f])
    assert sqr.locate(times, times[0] - 1e-9) == (-1, "before")
    assert sqr.locate(times, times[-1] + 1e-9) == (11, "after")
    assert sqr.locate(times, np.nextafter(times[3], np.inf)) == (3, "inside")
    assert sqr.locate(times, np.nextafter(times[4], -np.inf)) == (3, "inside")
    # the limit alpha -> 0 of the answer is the frame's own block
    t = times[2] + 1e-9 * (times[3] - times[2])
    near = sqr.block_form(z, times, S, R, t, SROT, STRANS)
    assert np.linalg.norm(near - S[2]) <= 1e-6 * np.linalg.norm(S[2])


def _refused(word, *a, **kw):
    with pytest.raises(aar.AarError) as e:
        aar.smooth_query_validate(*a, **kw)
    assert e.value.code == aar.AAR_ERR_INVALID and word in str(e.value), str(e.value)


def test_validate_messages():
    aar.smooth_query_validate(5, SROT, STRANS, [0.5, -3.0, 17.0, 0.5])
    aar.smooth_query_validate(5, SROT, STRANS, [])
    aar.smooth_query_validate(0, SROT, STRANS, [])
    aar.smooth_query_validate(1, SROT, STRANS, [2.0], frame_time=[1.0])
    _refused("query_time[2]", 5, SROT, STRANS, [0.0, 1.0, np.nan])
    _refused("query_time[0]", 5, SROT, STRANS, [np.inf])
    _refused("num_frames", 0, SROT, STRANS, [0.0])
    _refused("sigma_rot", 5, -1.0, STRANS, [0.0])
    _refused("frame_time[2]", 3, SROT, STRANS, [0.0], frame_time=[0.0, 1.0, 1.0])
    _refused("struct_size", 3, SROT, STRANS, [0.0], struct_size=8)
    with pytest.raises(aar.AarError) as e:
        aar._check(aar.lib().aar_smooth_query_validate(3, None, 0, None))
    assert e.value.code == aar.AAR_ERR_INVALID
    sp = aar.SmoothParams(SROT, STRANS)
    with pytest.raises(aar.AarError) as e:
        aar._check(aar.lib().aar_smooth_query_validate(3, C.byref(sp.c), 2, None))
    assert e.value.code == aar.AAR_ERR_INVALID and "query_time" in str(e.value)
    with pytest.raises(aar.AarError) as e:
        aar._check(aar.lib().aar_smooth_query_validate(3, C.byref(sp.c), -1, None))
    assert e.value.code == aar.AAR_ERR_INVALID and "n_query" in str(e.value)


def test_header_and_binding_declare_the_calls():
    with open(os.path.join(ROOT, "include", "aar.h")) as f:
        h = f.read()
    for n in ("aar_smooth_query_validate", "aar_track_smooth_query"):
        assert re.search(r"\bint\s+%s\s*\(" % n, h), n
        assert n in aar.SYMBOLS and hasattr(aar.lib(), n), n
    assert hasattr(aar.Problem, "track_smooth_query")
    m = re.search(r"typedef struct aar_smooth_query_report \{(.*?)\} aar_smooth_query_report;", h, re.S)
    assert m
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [k for k, _ in aar.CSmoothQueryReport._fields_]
    R = aar.CSmoothQueryReport
    assert C.sizeof(R) == 80
    assert [(k, getattr(R, k).offset) for k, _ in R._fields_] == [
        ("struct_size", 0), ("num_residuals", 8), ("num_vars", 16), ("data_cost", 24), ("prior_cost", 32), ("sigma2", 40), ("num_queries", 48),
        ("num_inside", 52), ("num_on_frame", 56), ("num_outside", 60), ("launches", 64), ("seconds", 72)]
    # rel_motion is refused in the header's words
    assert "rel_motion" in h[h.index("aar_smooth_query_report") - 4000:h.index("int aar_track_smooth_query")]
