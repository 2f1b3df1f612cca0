#!/usr/bin/env python3
"""Wall time of aar_track_smooth under the constant-velocity prior beside the random walk on the same inputs: the
tracking versions of configs 3, 4 and 5 (500 / 2000 / 5000 frames), from aar_track's result.  DESIGN.md section 16's method: 7 repeats after 2
warm-up calls, median (min ... max).  Per model: the call's wall time, report.seconds, the LM steps and rejected tries, the launches of one
damped solve.  Not part of bench.py.  Run on the MI355X:

    python scripts/smooth_cv_latency.py > profiles/smooth_cv_latency.txt

--package DIR takes the aar package of another build (DIR/aar, DIR/libaar.so) for an A/B run; one without the model runs the random walk alone.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SROT, STRANS = 0.05, 0.02
SROT0, STRANS0 = 1.0, 1.0
FRAMES = {3: 500, 4: 2000, 5: 5000}


def stats(t):
    t = 1e3 * np.asarray(t)
    return "%.3f ms (%.3f ... %.3f)" % (np.median(t), t.min(), t.max())


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    wall, inner = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        rep = fn()
        wall.append(time.perf_counter() - t0)
        inner.append(rep["seconds"])
    return wall, inner, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--package", default=os.path.join(ROOT, "automatic-ar_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import aar

    has_cv = hasattr(aar, "SMOOTH_MODEL_CONSTANT_VELOCITY")
    for cfg in a.configs:
        F = FRAMES[cfg]
        ds = aar.synth(cfg, num_frames=F)
        n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
        x0 = np.array(ds.x_full)
        x0[:n0] = ds.x_truth[:n0]
        with aar.Problem(ds) as p:
            xt, _, _ = p.track(x0, aar.lm_default_params())
            runs = [("random walk", {})]
            if has_cv:
                runs.append(("constant velocity", dict(model="cv", sigma_rot0=SROT0, sigma_trans0=STRANS0)))
            for name, kw in runs:
                wall, inner, rep = timed(lambda: p.track_smooth(xt, SROT, STRANS, **kw)[1], a.warmup, a.repeats)
                launches = "%d" % aar.smooth_solve_launches(F, kw.get("model", "rw")) if has_cv else "n/a"
                print("config %d, F = %d, %d detections, %s: aar_track_smooth %s, report.seconds %s, %d LM steps (%d rejected tries), "
                      "%s launches per solve, cost %.6f" % (cfg, F, ds.num_obs, name, stats(wall), stats(inner), rep["iterations"],
                                                            rep["rejected_tries"], launches, rep["final_cost"]), flush=True)


if __name__ == "__main__":
    main()
