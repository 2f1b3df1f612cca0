"""float64 restatement of the live tracker's gate (aar_tracker_enable_gate) -- TEST INFRASTRUCTURE ONLY.

Built on tests/track_restated.py and tests/live_restated.py (imported, not edited) and independent of csrc/live_gate_kernels.hip:

    e_d         sqrt((sum over the 4 corners of rx^2 + ry^2) / 4) of track_restated.residuals at the start pose z0, unweighted
    median      element floor((n - 1) / 2) of the ascending order, max the last; a non-finite e_d counts as +inf in both
    threshold   max(min_px, k_median median), k_median <= 0: min_px; fewer than min_detections detections: not gated, +inf, all kept
    keep        e_d <= threshold and e_d finite
    driver      GatedLive: gates every pushed frame at the pose its push starts from and feeds the kept rows to live_restated.Live
"""
import numpy as np

import live_restated as lr
import track_restated as tr


def det_err(fd, z0):
    """e_d [n] of a frame (track_restated's per-frame dict) at pose z0"""
    n = fd["ou"].shape[0]
    if n == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = tr.residuals(fd, np.asarray(z0, dtype=np.float64))          # [n, 4, 2]
        return np.sqrt(np.sum(r * r, axis=(1, 2)) / 4.0)


def rule(e, k_median, min_px, min_detections):
    """the rule on a list of errors: dict(gated, n_in, n_kept, n_nonfinite, median, max, threshold, keep [n] bool)"""
    e = np.asarray(e, dtype=np.float64).reshape(-1)
    n = len(e)
    fin = np.isfinite(e)
    key = np.sort(np.where(fin, e, np.inf))
    median = float(key[(n - 1) // 2]) if n else 0.0
    mx = float(key[-1]) if n else 0.0
    gated = n >= min_detections
    if not gated:
        thr, keep = np.inf, np.ones(n, dtype=bool)
    else:
        thr = max(float(min_px), float(k_median) * median) if k_median > 0 else float(min_px)
        with np.errstate(invalid="ignore"):
            keep = fin & (e <= thr)
    return dict(gated=int(gated), n_in=n, n_kept=int(keep.sum()), n_nonfinite=int((~fin).sum()), median=median, max=mx, threshold=float(thr), keep=keep)


def gate(fd, z0, k_median=6.0, min_px=3.0, min_detections=4):
    """(e_d [n], median, max, threshold, keep [n] bool) of a frame at its start pose"""
    e = det_err(fd, z0)
    g = rule(e, k_median, min_px, min_detections)
    return e, g["median"], g["max"], g["threshold"], g["keep"]


def select(fd, keep):
    """the frame's dict with the kept rows only, in order"""
    keep = np.asarray(keep, dtype=bool)
    return {k: v[keep] for k, v in fd.items()}


class _Frames:
    """what live_restated.Live reads of a TrackData: frame(f)"""

    def __init__(self):
        self.fds = []

    def frame(self, f):
        return self.fds[f]


class GatedLive:
    """push-by-push driver: push(fd, time, pose_init) gates the frame fd (a per-frame dict) at its start and pushes the kept rows"""

    def __init__(self, k_median=6.0, min_px=3.0, min_detections=4, **live_kw):
        self.rule_kw = dict(k_median=k_median, min_px=min_px, min_detections=min_detections)
        self.frames = _Frames()
        self.live = lr.Live(self.frames, **live_kw)

    def push(self, fd, time, pose_init=None):
        """Live.push's dict plus gate (rule()'s dict) and det_err"""
        z0 = np.asarray(pose_init, dtype=np.float64) if pose_init is not None else self.live.win[-1][2].copy()
        e = det_err(fd, z0)
        g = rule(e, **self.rule_kw)
        self.frames.fds.append(select(fd, g["keep"]))
        r = self.live.push(len(self.frames.fds) - 1, time, pose_init=pose_init)
        r.update(gate=g, det_err=e)
        return r
