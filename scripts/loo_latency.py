#!/usr/bin/env python3
"""Wall time of aar_problem_detection_loo beside aar_problem_detection_leverage (DESIGN.md sections 36, 37) in one process, at the start
points of synthetic configs 3 and 5, the two calls interleaved repeat by repeat; and at config 3 aar_problem_gate_detections for the
(camera, marker) pairs of one frame beside aar_problem_predict_corners with the covariance on the same queries.  DESIGN.md section 16's
method: 7 repeats after 2 warm-up calls, median (min ... max), host copies of the outputs included.  To tell the query kernel from the
copies of its outputs, detection_loo is also timed through the C ABI with EVERY output array NULL (the chain, the kernel, and the copies the
report itself needs: F, the leverage, status and keep -- 18 bytes per detection instead of 114) and with F and keep alone.  Not part of bench.py.
Run on the MI355X:

    python scripts/loo_latency.py > profiles/loo_latency.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
import aar  # noqa: E402


def stats(t):
    t = 1e3 * np.asarray(t)
    return "%.3f ms (%.3f ... %.3f)" % (np.median(t), t.min(), t.max())


def interleaved(fns, warmup, repeats):
    """the calls of fns in turn, repeat by repeat: one sitting, the same state of the machine for each"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            out[k].append(time.perf_counter() - t0)
    return out


def raw_loo(p, x, n, want):
    """a call of aar_problem_detection_loo through the C ABI that passes only the output arrays named in want"""
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    F, keep = np.empty(n), np.empty(n, dtype=np.uint8)
    args = [None, None, F.ctypes.data_as(dp) if "F" in want else None, None, None, None, None, keep.ctypes.data_as(bp) if "keep" in want else None]
    xp = x.ctypes.data_as(dp)

    def call():
        code = aar.lib().aar_problem_detection_loo(p.handle, xp, None, *args, None)
        assert code == aar.AAR_OK, aar.lib().aar_last_error()
    return call


def grid(ds, frames):
    c, m = np.meshgrid(np.arange(ds.num_cams), np.arange(ds.num_markers), indexing="ij")
    return np.concatenate([np.stack([c.reshape(-1), m.reshape(-1), np.full(c.size, f)], axis=1) for f in frames]).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    for cfg in a.configs:
        ds = aar.synth(cfg)
        x = np.asarray(ds.x_full, dtype=np.float64)
        with aar.Problem(ds) as p:
            loo = p.detection_loo(x)
            rep = loo.report
            t_lev, t_loo, t_null, t_fk = interleaved([lambda: p.detection_leverage(x), lambda: p.detection_loo(x), raw_loo(p, x, ds.num_obs, ()),
                                                      raw_loo(p, x, ds.num_obs, ("F", "keep"))], a.warmup, a.repeats)
            d = 1e3 * (np.median(t_loo) - np.median(t_lev))
            print("config %d (%d cameras, %d markers, %d frames, %d detections, %d unknowns, %d live): detection_leverage %s; detection_loo %s, "
                  "%d launches; difference of the medians %+.3f ms; %d undetermined, largest F %.3f, smallest margin %.3f" %
                  (cfg, ds.num_cams, ds.num_markers, ds.num_frames, ds.num_obs, p.num_vars, rep["predict"]["num_live_vars"], stats(t_lev), stats(t_loo),
                   rep["predict"]["launches"], d, rep["undetermined"], rep["max_f"], float(np.nanmin(loo.margin))), flush=True)
            print("config %d, detection_loo through the C ABI: every output NULL %s (%+.3f ms against detection_leverage); F and keep alone %s" %
                  (cfg, stats(t_null), 1e3 * (np.median(t_null) - np.median(t_lev)), stats(t_fk)), flush=True)
            if cfg != 3:
                continue
            q = grid(ds, [ds.num_frames // 2])
            uv, _, st, _ = p.predict_corners(x, q, covariance=False)
            obs = np.where(np.isfinite(uv.reshape(-1, 8)), uv.reshape(-1, 8) + 0.5, 0.0).astype(np.float32)
            g = p.gate_detections(x, q[:, 0], q[:, 1], q[:, 2], obs)[3]
            t_p, t_g = interleaved([lambda: p.predict_corners(x, q), lambda: p.gate_detections(x, q[:, 0], q[:, 1], q[:, 2], obs)], a.warmup, a.repeats)
            print("config %d, every (camera, marker) of one frame: %d queries (%d undefined, %d behind): predict_corners with cov %s; "
                  "gate_detections %s, %d launches" % (cfg, len(q), g["undefined"], g["behind"], stats(t_p), stats(t_g), g["launches"]), flush=True)


if __name__ == "__main__":
    main()
