"""Inputs of the tests of aar_track_smooth_relative (tests/test_smooth_relative_host.py, tests/test_gpu_track_smooth_relative.py) -- TEST
INFRASTRUCTURE ONLY."""
import numpy as np

import aar
import smooth_cases as sc
import smooth_cv_cases as cc
import smooth_fit_cases as fc

SROT, STRANS = cc.SROT, cc.STRANS
MODELS = {"rw": dict(model="rw"), "cv": dict(model="cv", sigma_rot0=cc.SROT0, sigma_trans0=cc.STRANS0)}
SIZES = [1, 2, 3, 4, 5, 8, 9, 33]          # odd and even, a chain of one step, the last supernode half filled
BIG = 515                                  # above 512: the levels of the reductions that get launches of their own


def dataset(F):
    """config 2 cut to F frames with the frames of smooth_cases.emptied(F) emptied"""
    ds = sc.without_frames(aar.synth(2, num_frames=F), sc.emptied(F))
    assert ds.num_frames == F
    return ds


def big_dataset():
    """BIG frames: smooth_fit_cases.shape_dataset (config 4 at that size, smooth_cases.emptied(BIG) emptied)"""
    ds = fc.shape_dataset(BIG)
    assert ds.num_frames == BIG
    return ds


def times(F):
    """uneven frame times (None for one frame)"""
    return cc.gaps(F) if F > 1 else None


def all_pairs(F):
    return np.array([(a, b) for a in range(F) for b in range(F)], dtype=np.int32).reshape(-1, 2)


def big_pairs():
    """64 fixed pairs of the BIG-frame problem: the longest lags, lags four and five on both supernode parities, both orders, every lag class"""
    F = BIG
    fixed = [(0, F - 1), (1, F - 1), (F - 1, 0), (F - 1, 1), (0, F - 2), (1, F - 2), (10, 14), (11, 15), (10, 15), (11, 16), (15, 10), (14, 10),
             (0, 0), (F - 1, F - 1), (7, 8), (8, 7), (7, 9), (8, 10), (7, 10), (8, 11), (11, 8), (F - 2, F - 1), (F - 3, F - 1), (F - 4, F - 1),
             (F - 5, F - 1), (F - 6, F - 1), (255, 256), (255, 257), (254, 258), (256, 512), (257, 513), (0, 256), (1, 257), (128, 384)]
    rng = np.random.default_rng(515)
    rest = rng.integers(0, F, size=(64 - len(fixed), 2))
    out = np.array(fixed + [tuple(int(v) for v in r) for r in rest], dtype=np.int32)
    assert out.shape == (64, 2)
    return out
