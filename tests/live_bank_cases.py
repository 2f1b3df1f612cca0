"""Inputs of the tracker bank tests (tests/test_gpu_live_bank.py) -- TEST INFRASTRUCTURE ONLY.

A bank member is a small synthetic solution of its own -- aar.synth(2, ...) cut down to the member's numbers of cameras and markers, 13 frames, a
handful of detections per frame (markers accepted up to a slant of acos 0.3, as tests/live_detection_cases.py does) -- with its own pattern of detection counts and of pushes that carry a pose_init.  Its pushes are restated by
tests/live_marginal_restated.py (LiveM: tests/live_restated.py's loop, fixed or marginalised anchor, covariance), once per (member, mode), shared.

Smallest restated margin over the six members and the pushes of each mode, measured on the CPU (PYTHONPATH=automatic-ar_amd python
tests/live_bank_cases.py; every slack is 0); every push the GPU tests use must stay above 1e-9, which compare_push asserts again:
    lag 0 smooth 0: 1.3e-04    lag 0 smooth 1: 2.1e-04    lag 1 fixed: 1.2e-06    lag 1 marginal: 2.8e-06    lag 3 fixed: 1.7e-06    lag 3 marginal: 1.6e-06
    raw detections (members 0 and 1, restated from the device's starts, lag 1; measured on the GPU): vote 3.7e-04, best 3.7e-04
"""
import functools
from types import SimpleNamespace

import numpy as np

import aar
import live_detection_cases as ld
import live_marginal_cases as mc
import live_marginal_restated as lm
import smooth_cases as sc
import track_restated as tr

SROT, STRANS = mc.SROT, mc.STRANS
N = 13                                   # 3 * (3 + 1) + 1 pushes: at lag 3 every ring slot row is used a third time, the first a fourth
TIMES = mc.times(N)
MODES = [(0, False), (0, True), (1, True), (3, True)]          # (lag, smooth)

# detections kept per frame (None: all the member has).  SHRINK: with 1, 2 and 4 ring slots every slot is reused by a frame with fewer and by one
# with more; SPECIAL: an empty frame and a one-detection frame that lie inside the window at lags 1 and 3
SHRINK = [None, 4, 3, 2, None, None, 3, 2, None, 1, 4, 2, 3]
SPECIAL = [None, None, None, 0, None, 1, None, None, 2, None, 0, None, None]
FIRST_EMPTY = [0] + [None] * 12          # the stream starts without detections: in marginal mode the first marginal is dropped
# init "even": a pose_init on pushes 0, 2, 4, ..., prediction on the others; "odd": the opposite (push 0 always has one)
SPECS = [dict(num_cams=4, num_markers=12, seed=11, counts=None, init="even"),
         dict(num_cams=3, num_markers=6, seed=12, counts=SHRINK, init="odd"),
         dict(num_cams=2, num_markers=5, seed=13, counts=SPECIAL, init="even"),
         dict(num_cams=4, num_markers=8, seed=14, counts=None, init="odd"),
         dict(num_cams=3, num_markers=9, seed=15, counts=SHRINK, init="even"),
         dict(num_cams=3, num_markers=4, seed=16, counts=FIRST_EMPTY, init="odd")]


@functools.lru_cache(maxsize=None)
def member(i):
    s = SPECS[i]
    ds = aar.synth(2, num_cams=s["num_cams"], num_markers=s["num_markers"], num_frames=N, seed=s["seed"], min_view_cos=0.3)
    x0 = sc.track_start(ds)
    if s["counts"] is not None:
        ds = mc.keep_first(ds, s["counts"])
    has_init = [f == 0 or (f % 2 == 0) == (s["init"] == "even") for f in range(N)]
    cnt = np.bincount(ds.obs_frame, minlength=N)
    return SimpleNamespace(name="m%d" % i, index=i, ds=ds, x0=x0, td=tr.TrackData(ds, x0), sol=sc.copy_of(ds, x_full=x0), has_init=has_init, cnt=cnt,
                           n=N, lag=None, frames=[mc.frame_obs(ds, f) for f in range(N)])


def pushes(lag):
    return 3 * (lag + 1) + 1


@functools.lru_cache(maxsize=None)
def restated(i, lag, smooth, anchor="fixed"):
    """every push of member i by LiveM (each dict also carries window and anchor after the push)"""
    m = member(i)
    live = lm.LiveM(m.td, lag=lag, smooth=smooth, sigma_rot=SROT, sigma_trans=STRANS, anchor=anchor)
    out = []
    for f in range(pushes(lag)):
        r = live.push(f, TIMES[f], pose_init=m.td.z0[f] if m.has_init[f] else None)
        r["window"], r["anchor"] = live.window()
        out.append(r)
    return out


def bank_kw(members, lag, smooth, **over):
    kw = dict(lag=lag, smooth=smooth, max_obs_per_frame=int(max(max(m.cnt.max() for m in members), 1)))
    if smooth:
        kw.update(sigma_rot=SROT, sigma_trans=STRANS)
    kw.update(over)
    return kw


def frames_of(members, f):
    return [m.frames[f] for m in members]


def inits_of(members, f):
    return [m.td.z0[f] if m.has_init[f] else None for m in members]


@functools.lru_cache(maxsize=None)
def tiny(k):
    """a neighbour for the crowded bank: 2 cameras, 4 markers, four detections per frame, its corners moved by noise of its own"""
    ds = aar.synth(2, num_cams=2, num_markers=4, num_frames=N, seed=100 + k % 5, min_view_cos=0.1)
    x0 = sc.track_start(ds)
    rng = np.random.default_rng(1000 + k)
    ds = sc.copy_of(ds, obs_uv=(np.array(ds.obs_uv) + rng.normal(0.0, 0.5, ds.obs_uv.shape)).astype(np.float32))
    cnt = np.bincount(ds.obs_frame, minlength=N)
    return SimpleNamespace(name="tiny%d" % k, ds=ds, x0=x0, td=tr.TrackData(ds, x0), sol=sc.copy_of(ds, x_full=x0), has_init=[f % 3 != 1 + k % 2 for f in range(N)],
                           cnt=cnt, n=N, frames=[mc.frame_obs(ds, f) for f in range(N)])


def noisy(m, k):
    """member m with other corners: a neighbour whose input differs from m's"""
    rng = np.random.default_rng(2000 + k)
    ds = sc.copy_of(m.ds, obs_uv=(np.array(m.ds.obs_uv) + rng.normal(0.0, 0.7, m.ds.obs_uv.shape)).astype(np.float32))
    return SimpleNamespace(name="%s-noisy%d" % (m.name, k), ds=ds, x0=m.x0, td=tr.TrackData(ds, m.x0), sol=m.sol, has_init=[not h or f == 0 for f, h in enumerate(m.has_init)],
                           cnt=m.cnt, n=N, frames=[mc.frame_obs(ds, f) for f in range(N)])


# ---- raw detections: three members on the scenes of tests/live_detection_cases.py ----
DET_PUSHES = 6


@functools.lru_cache(maxsize=None)
def det_members():
    """(scene, per-member detection keywords, frames [DET_PUSHES] of (cam, marker, raw uv)).  Member 2 alternates frames of ONE detection (one
    candidate: the second IPPE solution is never kept at threshold 1e-30) and of 65 detections (65 candidates)."""
    a, b = ld.case(False), ld.case(False, seed=77)
    one = ld.root_only_detection(a, 1)
    many = ld.pooled(a, 65)
    out = [(a, dict(Ks=a.K, dists=a.dists), [a.frames[f] for f in range(DET_PUSHES)]),
           (b, dict(Ks=b.K, dists=b.dists, ippe_threshold=1e30), [b.frames[f] for f in range(DET_PUSHES)]),
           (a, dict(Ks=a.K, dists=a.dists, ippe_threshold=1e-30, min_detections=1), [one if f % 2 == 0 else many for f in range(DET_PUSHES)])]
    return out


def margins():
    for lag, smooth in MODES:
        for anchor in (["fixed"] if lag == 0 else ["fixed", "marginal"]):
            worst = min(min(r["margin"] for r in restated(i, lag, smooth, anchor)) for i in range(len(SPECS)))
            slack = max(max(r["slack"] for r in restated(i, lag, smooth, anchor)) for i in range(len(SPECS)))
            print("lag %d smooth %d %s: smallest margin %.2e, largest slack %.2e" % (lag, smooth, anchor, worst, slack))
    for i in range(len(SPECS)):
        print("member %d: counts %s" % (i, list(member(i).cnt)))


if __name__ == "__main__":
    margins()
