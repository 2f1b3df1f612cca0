"""Generates the stored outputs of the real reference solver that tests/test_host_levmarq.py and
tests/test_oracle_golden.py::test_port_equals_live_reference_solver compare against.  Run where oracle/_ref is built
(python -c 'import __graft_entry__ as g; g.build()' with the reference sources present):

    python tests/golden/make_ref_vectors.py

g3_host_levmarq_ref.npz      -- per toy case of tests/test_host_levmarq.py (CASES): the real ucoslam::SparseLevMarq<double>'s
                                per-step error / damping / accepted flags, final error and final vector, with the case's arguments
g1_cfg3_cut_ref_threads2.npz -- the real solver on g1_cfg3_cut.npz from its initial guess, default parameters, 2 threads:
                                final vector, iterations, final error
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "automatic-ar_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import oracle_lib as ol  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_host_levmarq import CASES, REF_KEYS, ref_toy_live  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    assert ol.have_ref(), "build oracle/_ref first (python -c 'import __graft_entry__ as g; g.build()')"
    out = {}
    for i, (name, args) in enumerate(CASES):
        r = ref_toy_live(*args)
        for k in REF_KEYS:
            out["case%d_%s" % (i, k)] = np.atleast_1d(np.asarray(r[k]))
        out["case%d_args" % i] = np.array(args, dtype=np.float64)
        print(name, "steps", len(r["err"]), "final_err", r["final_err"])
    np.savez_compressed(os.path.join(OUT, "g3_host_levmarq_ref.npz"), **out)

    ds, _ = load_golden("g1_cfg3_cut")
    x, rep = ol.Oracle(ds).ref_lm_solve(ds.x_full, threads=2)
    np.savez_compressed(os.path.join(OUT, "g1_cfg3_cut_ref_threads2.npz"), x=x, iterations=np.array([rep["iterations"]]),
                        final_err=np.array([rep["final_err"]]))
    print("g1_cfg3_cut threads 2: iterations", rep["iterations"], "final_err", rep["final_err"])
