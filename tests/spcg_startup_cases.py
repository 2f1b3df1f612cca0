"""The shapes of tests/test_gpu_spcg_startup.py, shared with scripts/record_spcg_startup_golden.py (which wrote tests/golden/spcg_startup_parent.npz from
the build BEFORE k_spcg's set-up was reworked): the smallest problems at which the set-up of k_spcg<NT, CO> takes each of its paths.

Every case is aar.synth(3, num_cams, num_markers, num_frames=30), solver "spcg", deterministic (S is the same bits in every run; k_spcg itself has no
atomics), one eval_damped_step at the start point at the LM run's first mu (tau max diag H) and at a mu one thousand times smaller."""
import contextlib
import os

import numpy as np

import aar

# name -> (cameras, markers, entities fixed by the caller beyond the roots)
CASES = {
    "nt1_16": (4, 12, False),            # NT = 1, no padding entity
    "nt2_30": (6, 24, False),            # NT = 2, two padding entities
    "nt3_48": (8, 40, False),            # NT = 3, no padding
    "nt3_40": (8, 32, False),            # NT = 3, eight identity-row entities
    "nt4_60": (8, 52, False),            # NT = 4
    "nt5_70": (8, 62, False),            # NT = 5: the mask of fixed entities crosses a 64-bit word
    "nt3_48_fixed": (8, 40, True),       # one more camera and one more marker held fixed
}
GOLDEN_FILE = "spcg_startup_parent.npz"


def key(name, coarse):
    return "%s_%s" % (name, "co" if coarse else "bj")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dataset(name):
    C, M, _ = CASES[name]
    return aar.synth(3, num_cams=C, num_markers=M, num_frames=30)


def fixed_sets(ds, name):
    """the two entities of case `name` that the caller holds fixed (neither is a root)"""
    if not CASES[name][2]:
        return {}
    cam = next(c for c in range(ds.num_cams) if c != ds.root_cam and c >= 2)
    marker = next(m for m in range(ds.num_markers) if m != ds.root_marker and m >= 5)
    return dict(fixed_cams=[cam], fixed_markers=[marker])


def run(name, coarse, mus=None):
    """(mu [2], delta [2][num_vars], last_iterations [2], fallbacks) of the two one-off steps; mus: take these dampings instead of the run's own"""
    ds = dataset(name)
    # the library reads its switches when the problem is created
    with _env(AAR_SPCG_COARSE_FROM="0" if coarse else "100000"):
        p = aar.Problem(ds, solver="spcg", deterministic=True, **fixed_sets(ds, name))
    with p:
        assert p.solver_stats()["solver"] == "spcg"
        x0 = np.asarray(ds.x_full, dtype=np.float64)
        if mus is None:
            H0, _, _ = p.eval_normal_equations(x0)
            mu0 = aar.lm_default_params().tau * float(np.diag(H0).max())
            mus = np.array([mu0, mu0 * 1e-3])
        deltas, its = [], []
        for mu in mus:
            deltas.append(p.eval_damped_step(x0, float(mu)))
            its.append(p.solver_stats()["last_iterations"])
        fb = p.solver_stats()["fallbacks"]
    return np.asarray(mus, dtype=np.float64), np.stack(deltas), np.asarray(its, dtype=np.int64), int(fb)
