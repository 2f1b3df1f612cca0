#!/usr/bin/env python3
"""Wall time of aar_track_smooth_relative on the tracking versions of configs 3, 4 and 5 (500 / 2000 / 5000 frames), under
both motion models, at aar_track_smooth's result started from aar_track's, for two sets of pairs:
  - every frame relative to frame 0 (F pairs, lags 0 .. F - 1);
  - 5000 random pairs (seed 35).
Beside it, on the same inputs, aar_track_smooth_covariance2 alone, whose chain the call contains: the difference is the cost of the gains and
the queries.  DESIGN.md section 16's method: 7 repeats after 2 warm-up calls, median (min ... max).  Not part of bench.py.  Run on the MI355X:

    python scripts/smooth_relative_latency.py > profiles/smooth_relative.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "automatic-ar_amd"))
import aar  # noqa: E402

SROT, STRANS = 0.05, 0.02
MODELS = {"rw": dict(model="rw"), "cv": dict(model="cv", sigma_rot0=1.0, sigma_trans0=1.0)}
FRAMES = {3: 500, 4: 2000, 5: 5000}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--random", type=int, default=5000, help="random pairs")
    a = ap.parse_args()
    for cfg in a.configs:
        F = FRAMES[cfg]
        ds = aar.synth(cfg, num_frames=F)
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        to_zero = np.stack([np.zeros(F, dtype=np.int32), np.arange(F, dtype=np.int32)], 1)
        rnd = np.random.default_rng(35).integers(0, F, size=(a.random, 2)).astype(np.int32)
        for name, kw in MODELS.items():
            with aar.Problem(ds) as p:
                xt, _, _ = p.track(x0, aar.lm_default_params())
                xs = p.track_smooth(xt, SROT, STRANS, **kw)[0]
                r0 = p.track_smooth_relative(xs, SROT, STRANS, to_zero, **kw)[3]
                r1 = p.track_smooth_relative(xs, SROT, STRANS, rnd, **kw)[3]
                t_0 = timed(lambda: p.track_smooth_relative(xs, SROT, STRANS, to_zero, **kw), a.warmup, a.repeats)
                t_r = timed(lambda: p.track_smooth_relative(xs, SROT, STRANS, rnd, **kw), a.warmup, a.repeats)
                t_c = timed(lambda: p.track_smooth_covariance2(xs, SROT, STRANS, lag2=name == "cv", **kw), a.warmup, a.repeats)
            print("config %d, F = %d, %d detections, %s: every frame relative to frame 0 (%d pairs, %d chained, longest lag %d) %s, %d launches; "
                  "%d random pairs (%d chained, longest lag %d, mean lag %.0f) %s, %d launches; aar_track_smooth_covariance2 alone %s" %
                  (cfg, F, ds.num_obs, name, F, r0["num_chained"], r0["max_lag"], stats(t_0), r0["launches"], len(rnd), r1["num_chained"],
                   r1["max_lag"], float(np.mean(np.abs(rnd[:, 0] - rnd[:, 1]))), stats(t_r), r1["launches"], stats(t_c)), flush=True)


if __name__ == "__main__":
    main()
