"""The numpy restatement of the selected inverse (tests/smooth_covariance_restated.py) against numpy.linalg.inv of the dense matrix, on systems of
tests/smooth_restated.py, and the interface of aar_track_smooth_covariance as header and binding declare it.  CPU only.

Bar: largest entry error of the selected blocks over their largest entry <= 0.5 eps kappa_2(H): ten times what the recursion reached on random
block-tridiagonal systems when it was designed (0.05 eps kappa_2), and a twentieth of the device test's bar."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_covariance_restated as scr
import smooth_restated as sr
import track_restated as tr
from conftest import ROOT, load_golden

EPS = np.finfo(np.float64).eps
SROT, STRANS = 0.05, 0.02
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 127]


def _gaps(F):
    return np.cumsum(np.r_[0.0, 1.0 + (np.arange(F - 1) % 7 == 3) * 4.0])


_BASE = {}


def _base(name):
    """(data set, start) of the two golden inputs, loaded once"""
    if name not in _BASE:
        ds, g = load_golden(name)
        if name == "g_track_cfg2":
            ds.x_full = np.array(g["track_x0"])
        _BASE[name] = ds
    return _BASE[name]


def _resized(ds, F):
    """the data set at F frames: frame f is the base's frame f mod its frame count, detections and start pose with it"""
    F0 = ds.num_frames
    if F == F0:
        return ds
    n0 = sc.ns(ds)
    x = np.array(ds.x_full)
    src = np.arange(F) % F0
    by_frame = [np.nonzero(np.asarray(ds.obs_frame) == f)[0] for f in range(F0)]
    sel = np.concatenate([by_frame[f] for f in src])
    frame = np.concatenate([np.full(len(by_frame[f]), k, dtype=np.asarray(ds.obs_frame).dtype) for k, f in enumerate(src)])
    z = x[n0:n0 + 6 * F0].reshape(F0, 6)[src].reshape(-1)
    return sc.copy_of(ds, num_frames=F, frame_ids=np.arange(F, dtype=np.int32), obs_frame=frame, obs_cam=ds.obs_cam[sel],
                      obs_marker=ds.obs_marker[sel], obs_uv=ds.obs_uv[sel], x_full=np.concatenate([x[:n0], z, x[n0 + 6 * F0:]]))


def _system(name, F, variant):
    """(diag, off) of the F-frame problem with the frames of sc.emptied(F) emptied"""
    ds = sc.without_frames(_resized(_base(name), F), sc.emptied(F))
    x0 = np.array(ds.x_full)
    ft = _gaps(F) if "gaps" in variant and F > 1 else None
    rng = np.random.default_rng(3)
    rel = rng.normal(size=(F - 1, 6)) * [0.05, 0.05, 0.05, 0.02, 0.02, 0.02] if "rel" in variant and F > 1 else None
    td = tr.TrackData(ds, x0)
    sp = sr.SmoothProblem(td, SROT, STRANS, frame_time=ft, rel_motion=rel)
    diag, off, _ = sp.system(td.z0)
    return diag, off


@pytest.mark.parametrize("variant", ["plain", "gaps_rel"])
@pytest.mark.parametrize("F", SIZES)
@pytest.mark.parametrize("name", ["g2_small", "g_track_cfg2"])
def test_restated_recursion_against_the_dense_inverse(name, F, variant):
    diag, off = _system(name, F, variant)
    assert diag.shape[0] == F
    H = sr.dense(diag, off)
    Sd, Rd = scr.selected_blocks(np.linalg.inv(H), F)
    S, R = scr.selected_inverse(diag, off)
    kappa = np.linalg.cond(H)
    e_s = np.abs(S - Sd).max() / np.abs(Sd).max()
    e_r = np.abs(R - Rd).max() / np.abs(Rd).max() if F > 1 else 0.0
    print("%s F %d %s: kappa %.2e, frame %.2e lag %.2e (in eps kappa: %.3f %.3f), block rows %.2e" %
          (name, F, variant, kappa, e_s, e_r, e_s / (EPS * kappa), e_r / (EPS * kappa), scr.block_row_residual(diag, off, S, R)))
    assert e_s <= 0.5 * EPS * kappa and e_r <= 0.5 * EPS * kappa, (e_s, e_r, EPS * kappa)
    assert np.array_equal(S, np.swapaxes(S, 1, 2))


def test_block_row_residual_sees_a_wrong_block():
    diag, off = _system("g_track_cfg2", 5, "plain")
    S, R = scr.selected_inverse(diag, off)
    good = scr.block_row_residual(diag, off, S, R)
    assert good < 1e-12
    for k in range(4):
        Rb = R.copy()
        Rb[k] = Rb[k].T * 1.001
        assert scr.block_row_residual(diag, off, S, Rb) > 1e6 * good
    Sb = S.copy()
    Sb[2] *= 1.0 + 1e-6
    assert scr.block_row_residual(diag, off, Sb, R) > 1e6 * good


def test_prior_alone_is_refused():
    ds = sc.without_frames(aar.synth(2, num_frames=6), range(6))
    td = tr.TrackData(ds, sc.track_start(ds))
    diag, off, _ = sr.SmoothProblem(td, SROT, STRANS).system(td.z0)
    with pytest.raises(scr.NotPositive):
        scr.selected_inverse(diag, off)


def test_header_and_binding_declare_the_call():
    with open(os.path.join(ROOT, "include", "aar.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+aar_track_smooth_covariance\s*\(", h)
    assert "aar_track_smooth_covariance" in aar.SYMBOLS
    m = re.search(r"typedef struct aar_smooth_covariance_report \{(.*?)\} aar_smooth_covariance_report;", h, re.S)
    assert m
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [k for k, _ in aar.CSmoothCovarianceReport._fields_]
    assert C.sizeof(aar.CSmoothCovarianceReport) == 64
    assert hasattr(aar.lib(), "aar_track_smooth_covariance") and hasattr(aar.Problem, "track_smooth_covariance")
