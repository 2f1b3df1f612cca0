"""k_spcg's set-up (csrc/spcg_kernels.hip: the mask of fixed entities in the kernel arguments, the rows of S read in 16-byte pieces)
computes what the set-up before it computed, to the last bit.  Needs a real MI355X.

tests/golden/spcg_startup_parent.npz was recorded by scripts/record_spcg_startup_golden.py from the build of the commit before the rework; the cases
(tests/spcg_startup_cases.py) are the smallest shapes at which the set-up takes each of its paths, each with block-Jacobi (k_spcg<NT, false>) and with
the coarse space forced on (k_spcg<NT, true>).  With deterministic=True the reduced system S is the same bits in every run and k_spcg has no atomics, so
a solve returns the same bits for the same S: any difference is a changed operation or a changed order.
"""
import os

import numpy as np
import pytest

import aar
import spcg_startup_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, sc.GOLDEN_FILE)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("coarse", [False, True], ids=["block_jacobi", "coarse"])
@pytest.mark.parametrize("name", list(sc.CASES))
def test_step_equals_the_parent_builds_bits(name, coarse, golden):
    k = sc.key(name, coarse)
    mus, d, its, fb = sc.run(name, coarse, mus=golden[k + "_mu"])
    g = golden[k + "_delta"]
    print("%s: iterations %s (golden %s), fall-backs %d, differing entries %d of %d, max |diff| %.3e"
          % (k, its.tolist(), golden[k + "_its"].tolist(), fb, int((_bits(d) != _bits(g)).sum()), d.size, np.abs(d - g).max()))
    assert fb == 0                                          # (c)
    assert np.array_equal(its, golden[k + "_its"])          # (a) the same iteration counts ...
    assert d.shape == g.shape and np.array_equal(_bits(d), _bits(g))   # ... and the same bits
    assert np.abs(d).max() > 0.0
