#!/usr/bin/env python3
"""Writes tests/golden/spcg_startup_parent.npz: for every case of tests/spcg_startup_cases.py, with block-Jacobi and with the coarse space forced on, the
two dampings, the two steps of eval_damped_step and their CG iteration counts, as the build in the tree computes them on the GPU.

It was run ONCE, on the commit before k_spcg's set-up was reworked; tests/test_gpu_spcg_startup.py holds every later build to those bits.  Running it
again on a later build would only record that build against itself.

    python scripts/record_spcg_startup_golden.py [--out FILE] [--compare]      (--compare: write nothing, report how the build differs from the file)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "automatic-ar_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import aar  # noqa: E402
import spcg_startup_cases as sc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", sc.GOLDEN_FILE))
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    if aar.device_count() < 1:
        sys.exit("no HIP device")
    old = dict(np.load(a.out)) if a.compare else None
    out, bad = {}, 0
    for name in sc.CASES:
        for coarse in (False, True):
            k = sc.key(name, coarse)
            mus, d, its, fb = sc.run(name, coarse, mus=old[k + "_mu"] if old else None)
            print("%-22s mu %.6e %.6e  iterations %s  fallbacks %d" % (k, mus[0], mus[1], its.tolist(), fb), flush=True)
            if old:
                same = np.array_equal(d.view(np.int64), old[k + "_delta"].view(np.int64)) and np.array_equal(its, old[k + "_its"])
                print("    against the file: %s (max |diff| %.3e)" % ("equal bits" if same else "DIFFERENT", np.abs(d - old[k + "_delta"]).max()), flush=True)
                bad += 0 if same else 1
            if fb:
                sys.exit("%s: %d fall-backs: not a case the golden file can hold" % (k, fb))
            out[k + "_mu"], out[k + "_delta"], out[k + "_its"] = mus, d, its
    if a.compare:
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
