"""The numpy restatement of the constant-velocity selected inverse (tests/smooth_cv_covariance_restated.py: the recursion of DESIGN.md section
32 on 12x12 supernodes) against numpy.linalg.inv of the dense matrix, on systems of tests/smooth_cv_restated.py, and the interface of
aar_track_smooth_covariance2 as header and binding declare it.  CPU only.

Bar (frame_cov, lag_cov, lag2_cov alike): largest entry error over the largest entry of the yardstick's selected blocks <= 10 eps kappa_2(H),
the forward-error order of any inverse (section 28's bar).  The yardstick itself is held to the same bar against long-double iterative
refinement of a few of its columns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_covariance_restated as scr
import smooth_cv_cases as cc
import smooth_cv_covariance_restated as ccr
import smooth_cv_restated as cv
import track_restated as tr
from conftest import ROOT

EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 66, 129, 131]

_SYS = {}


def _system(F):
    """(diag, off, off2) of config 2 cut to F frames, the frames of sc.emptied(F) emptied, on uneven frame times"""
    if F not in _SYS:
        ds = sc.without_frames(aar.synth(2, num_frames=F), sc.emptied(F))
        td = tr.TrackData(ds, sc.track_start(ds))
        sp = cv.SmoothCvProblem(td, cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0, frame_time=cc.gaps(F) if F > 1 else None)
        _SYS[F] = sp.system(td.z0)[:3]
    return _SYS[F]


def _refined_columns(H, Hi, cols):
    """long-double iterative refinement of the columns `cols` of the inverse Hi of H"""
    Hl = H.astype(np.longdouble)
    X = Hi[:, cols].astype(np.longdouble)
    E = np.eye(H.shape[0], dtype=np.longdouble)[:, cols]
    for _ in range(3):
        r = (E - Hl @ X).astype(np.float64)
        X = X + np.linalg.solve(H, r)
    return X


@pytest.mark.parametrize("F", SIZES)
def test_restated_recursion_against_the_dense_inverse(F):
    diag, off, off2 = _system(F)
    assert diag.shape[0] == F and (F < 3 or np.abs(off2).max() > 0)
    H = cv.dense(diag, off, off2)
    Hi = np.linalg.inv(H)
    kappa = np.linalg.cond(H)
    bar = 10 * EPS * kappa
    cols = sorted(set(int(c) for c in (0, 5, 6 * (F // 3) + 2, 6 * (F // 2) + 3, 6 * F - 6, 6 * F - 1) if 0 <= c < 6 * F))
    X = _refined_columns(H, Hi, cols)
    e_y = float(np.abs(Hi[:, cols] - X).max() / np.abs(X).max())
    assert e_y <= bar, ("the yardstick itself", e_y, bar)
    want = ccr.selected_blocks(Hi, F)
    got = ccr.selected_inverse(diag, off, off2)
    big = max(np.abs(w).max() for w in want if w.size)
    errs = [float(np.abs(g - w).max() / big) if w.size else 0.0 for g, w in zip(got, want)]
    rows = ccr.block_row_residual(diag, off, off2, *got)
    print("F %d: kappa %.2e, yardstick %.2e, frame %.2e lag %.2e lag2 %.2e (in eps kappa: %.2e %.2e %.2e), block rows %.2e (numpy %.2e)" %
          ((F, kappa, e_y) + tuple(errs) + tuple(e / (EPS * kappa) for e in errs) + (rows, ccr.block_row_residual(diag, off, off2, *want))))
    assert [g.shape for g in got] == [(F, 6, 6), (max(F - 1, 0), 6, 6), (max(F - 2, 0), 6, 6)]
    assert max(errs) <= bar, (errs, bar)
    assert np.array_equal(got[0], np.swapaxes(got[0], 1, 2))


def test_no_frames():
    z = np.zeros((0, 6, 6))
    assert [g.shape for g in ccr.selected_inverse(z, z, z)] == [(0, 6, 6)] * 3


@pytest.mark.parametrize("F", [1, 6, 7])
def test_prior_alone_trips_the_root_rule(F):
    ds = sc.without_frames(aar.synth(2, num_frames=F), range(F))
    assert ds.num_obs == 0
    td = tr.TrackData(ds, sc.track_start(ds))
    diag, off, off2, _ = cv.SmoothCvProblem(td, cc.SROT, cc.STRANS, cc.SROT0, cc.STRANS0).system(td.z0)
    with pytest.raises(scr.NotPositive):
        ccr.selected_inverse(diag, off, off2)


@pytest.mark.parametrize("F", [2, 5, 6])
def test_unpacking_table_on_distinct_entries(F):
    """S[k], R[k] cut from a symmetric matrix whose entries are all different: the unpacked blocks are that matrix's selected blocks"""
    n = 6 * F
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    M = (1000.0 * np.minimum(i, j) + np.maximum(i, j) + 1.0)
    assert len(np.unique(np.triu(M)[np.triu_indices(n)])) == n * (n + 1) // 2
    K = (F + 1) // 2
    P = np.full((12 * K, 12 * K), np.nan)           # the padded frame of an odd F: anything read from it shows as NaN
    P[:n, :n] = M
    S = np.stack([P[12 * k:12 * k + 12, 12 * k:12 * k + 12] for k in range(K)])
    R = np.stack([P[12 * k:12 * k + 12, 12 * k + 12:12 * k + 24] if k + 1 < K else np.full((12, 12), np.nan) for k in range(K)])
    got = ccr.unpack(S, R, F)
    for g, w in zip(got, ccr.selected_blocks(M, F)):
        assert g.shape == w.shape and np.array_equal(g, w)


def test_block_row_residual_sees_a_wrong_block():
    diag, off, off2 = _system(7)
    S, R, R2 = ccr.selected_inverse(diag, off, off2)
    good = ccr.block_row_residual(diag, off, off2, S, R, R2)
    assert good < 1e-12
    for k in range(5):
        bad = R2.copy()
        bad[k] = bad[k].T * 1.001
        assert ccr.block_row_residual(diag, off, off2, S, R, bad) > 1e6 * good
    bad = R.copy()
    bad[3] *= 1.001
    assert ccr.block_row_residual(diag, off, off2, S, bad, R2) > 1e6 * good


def test_header_and_binding_declare_the_call():
    with open(os.path.join(ROOT, "include", "aar.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+aar_track_smooth_covariance2\s*\(", h)
    assert "aar_track_smooth_covariance2" in aar.SYMBOLS
    assert hasattr(aar.lib(), "aar_track_smooth_covariance2") and hasattr(aar.Problem, "track_smooth_covariance2")
    assert len(aar.lib().aar_track_smooth_covariance2.argtypes) == 7
    assert C.sizeof(aar.CSmoothCovarianceReport) == 64
