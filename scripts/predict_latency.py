#!/usr/bin/env python3
"""Wall time of aar_problem_detection_leverage and aar_problem_predict_corners at the start points of the synthetic
configs:
  - the leverage of every detection at configs 3 and 5;
  - predict_corners for every (camera, marker) of ONE frame and of EVERY frame at config 3, with the covariance and without (cov = NULL: no
    covariance chain);
  - on the same inputs aar_problem_covariance alone (diagonal blocks and frame blocks), whose chain the calls contain: the difference is what
    the gains launch, the query kernel and the copies of the outputs add.
DESIGN.md section 16's method: 7 repeats after 2 warm-up calls, median (min ... max), host copies of the outputs included.  Not part of bench.py.
Run on the MI355X:

    python scripts/predict_latency.py > profiles/predict_latency.txt
"""
import argparse
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


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


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
            lev, _, rep = p.detection_leverage(x)
            t_l = timed(lambda: p.detection_leverage(x), a.warmup, a.repeats)
            t_c = timed(lambda: p.covariance(x, dense=False), a.warmup, a.repeats)
            print("config %d (%d cameras, %d markers, %d frames, %d detections, %d unknowns, %d live): detection_leverage %s, %d launches, sum of "
                  "leverages %.6f, largest %.3f; aar_problem_covariance alone %s" %
                  (cfg, ds.num_cams, ds.num_markers, ds.num_frames, ds.num_obs, p.num_vars, rep["num_live_vars"], stats(t_l), rep["launches"],
                   rep["leverage_sum"], float(np.nanmax(lev)), stats(t_c)), flush=True)
            if cfg != 3:
                continue
            for name, q in (("one frame", grid(ds, [ds.num_frames // 2])), ("every frame", grid(ds, range(ds.num_frames)))):
                r1 = p.predict_corners(x, q)[3]
                r0 = p.predict_corners(x, q, covariance=False)[3]
                t_1 = timed(lambda: p.predict_corners(x, q), a.warmup, a.repeats)
                t_0 = timed(lambda: p.predict_corners(x, q, covariance=False), a.warmup, a.repeats)
                print("config %d, predict_corners, every (camera, marker) of %s: %d queries (%d undefined, %d behind): with cov %s, %d launches; "
                      "cov = NULL %s, %d launches" % (cfg, name, len(q), r1["undefined"], r1["behind"], stats(t_1), r1["launches"], stats(t_0),
                                                       r0["launches"]), flush=True)


if __name__ == "__main__":
    main()
