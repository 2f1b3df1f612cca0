"""Inputs of the gate tests (tests/test_live_gate_host.py, tests/test_gpu_live_gate.py) -- TEST INFRASTRUCTURE ONLY.

The scene is tests/live_detection_cases.py's (4 cameras, 8 markers, 12 frames, 0.2 px).  Planted outliers, the everyday failures of marker tracking:

    id       a misread id: the detection's marker index replaced by another marker's
    rot      the corner order rotated by one
    shift    all four corners shifted by 40 px

(A rotated corner order is off by about the marker's side in the image, some 30 to 60 px here: the rule catches it where that exceeds the threshold,
so under a poor start -- k_median * median of 30 px and more -- it may stay.  The streams' plan is such that at the starts the raw-detection tests
meet, the vote's, every planted outlier is beyond the threshold and every inlier within; the tests assert it.)

Single frames (frames()): every size at which the kernel takes another path -- n = 3 (below min_detections), 4, an odd and an even n, duplicated
detections that tie at the median, 300 (more than one record per thread's chunk, outliers among the first ten so that kept records move across chunk
boundaries) and 4096 (every odd record an outlier under a fixed threshold) -- at two starts: the truth, and the truth perturbed by (0.02 rad, 0.01 m),
where the inliers are several pixels off and k_median * median decides.  The start from the previous estimate is a matter of streams (stream()).

margin(e, g) is the condition under which keep flags and the median's position cannot depend on rounding: no e_d within a relative 1e-6 of the
threshold, and the e_d on either side of the median position either equal or further apart than that.  tests/test_live_gate_host.py asserts it
for every case here with the restated e_d; seeds and shifts were picked so that it holds.
"""
import functools
from types import SimpleNamespace

import numpy as np

import live_detection_cases as ld
import live_gate_restated as gr

MARGIN = 1e-6
DEFAULT = dict(k_median=6.0, min_px=3.0, min_detections=4)
FIXED = dict(k_median=0.0, min_px=3.0, min_detections=4)          # a fixed threshold of 3 px
EMPTYING = dict(k_median=-1.0, min_px=1e-3, min_detections=4)     # nothing survives a gated frame
SHIFT = 40.0
D_ROT = 0.02 * np.array([0.6, -0.64, 0.48])
D_TRANS = 0.01 * np.array([-0.48, 0.6, 0.64])


def scene():
    return ld.case(False)


def truth(f):
    c = scene()
    return np.array(c.ds.x_truth[c.ns + 6 * f:][:6], dtype=np.float64)


def perturbed(f):
    return truth(f) + np.r_[D_ROT, D_TRANS]


def plant(cam, mk, uv, what):
    """(cam, mk, uv) with the outliers of `what` = [(index, kind)] planted; also the planted mask"""
    c = scene()
    cam, mk, uv = np.array(cam, dtype=np.int32), np.array(mk, dtype=np.int32), np.array(uv, dtype=np.float32).reshape(-1, 8)
    bad = np.zeros(len(cam), dtype=bool)
    for i, kind in what:
        assert not bad[i]
        bad[i] = True
        if kind == "id":
            mk[i] = (mk[i] + 3) % c.ds.num_markers
        elif kind == "rot":
            uv[i] = np.roll(uv[i].reshape(4, 2), 1, axis=0).reshape(8)
        elif kind == "shift":
            uv[i] = uv[i] + np.float32(SHIFT)
        else:
            raise ValueError(kind)
    return cam, mk, uv, bad


def synthetic(n, f, seed):
    """n detections of the camera / marker pairs the scene saw, all at frame f's true pose, 0.2 px"""
    c = scene()
    cam, mk, _ = ld.pooled(c, n)
    uv = ld.project(c, cam, mk, truth(f), noise=0.2, rng=np.random.default_rng(seed))
    assert np.all(np.isfinite(uv)) and np.abs(uv).max() < 1e5
    return cam, mk, uv


@functools.lru_cache(maxsize=None)
def frames():
    """the single-frame cases: name -> namespace(cam, mk, uv, bad, z0, rule, fd, e, g)"""
    c = scene()
    out = {}

    def add(name, cam, mk, uv, bad, z0, rule):
        fd = ld.frame_data(c, cam, mk, uv)
        e = gr.det_err(fd, z0)
        out[name] = SimpleNamespace(name=name, cam=cam, mk=mk, uv=uv, bad=bad, z0=np.array(z0), rule=dict(rule), fd=fd, e=e, g=gr.rule(e, **rule))

    for start, zf in (("truth", truth), ("pert", perturbed)):
        cam, mk, uv = c.frames[2]
        n = len(cam)
        assert n >= 9
        add("n3-" + start, *plant(cam[:3], mk[:3], uv[:3], [(1, "shift")]), zf(2), DEFAULT)
        add("n4-" + start, *plant(cam[:4], mk[:4], uv[:4], [(2, "id")]), zf(2), DEFAULT)
        odd, even = (n, n - 1) if n % 2 else (n - 1, n)
        add("odd-" + start, *plant(cam[:odd], mk[:odd], uv[:odd], [(1, "id"), (4, "rot")]), zf(2), DEFAULT)
        add("even-" + start, *plant(cam[:even], mk[:even], uv[:even], [(0, "rot"), (3, "shift"), (6, "id")]), zf(2), DEFAULT)
        # every detection twice: the two e_d around the median position are the same detection's
        m = 5
        dup = np.repeat(np.arange(m), 2)
        add("ties-" + start, *plant(cam[dup], mk[dup], uv[dup], [(9, "shift")]), zf(2), DEFAULT)
        cam, mk, uv = synthetic(300, 5, 11)
        add("n300-" + start, *plant(cam, mk, uv, [(1, "id"), (4, "rot"), (7, "shift"), (9, "shift"), (130, "rot"), (257, "shift"), (299, "id")]), zf(5), DEFAULT)
    cam, mk, uv = synthetic(4096, 7, 13)
    add("n4096-odd", *plant(cam, mk, uv, [(i, "shift") for i in range(1, 4096, 2)]), truth(7), FIXED)
    cam, mk, uv = c.frames[3]
    nan = np.array(uv)
    nan[2, 5] = np.nan
    nan[4, 0] = np.inf
    bad = np.zeros(len(cam), dtype=bool)
    bad[[2, 4]] = True
    add("nonfinite", cam, mk, nan, bad, truth(3), DEFAULT)
    add("empty", cam, mk, uv, np.zeros(len(cam), dtype=bool), truth(3), EMPTYING)
    return out


def margin(e, g):
    """True when no rounding of e_d can change the keep flags or the median's value by more than rounding"""
    e = np.asarray(e, dtype=np.float64)
    fin = np.isfinite(e)
    t = g["threshold"]
    if g["gated"] and np.isfinite(t) and np.any(np.abs(e[fin] - t) <= MARGIN * max(t, 1e-300)):
        return False
    key = np.sort(np.where(fin, e, np.inf))
    n, m = len(key), (len(key) - 1) // 2
    for a, b in ((m - 1, m), (m, m + 1)):
        if a < 0 or b >= n or key[a] == key[b] or not np.isfinite(key[b]):
            continue
        if key[b] - key[a] <= MARGIN * key[b]:
            return False
    return True


# ---- streams ----
PLAN = {0: [(1, "id")], 1: [(2, "rot"), (5, "shift")], 2: [], 3: [(0, "shift")], 4: [(3, "id"), (6, "shift")], 5: [(2, "shift")],
        6: [(0, "id")], 7: [], 8: [(1, "rot")], 9: [(5, "id"), (7, "shift")], 10: [(3, "rot")], 11: [(4, "shift")]}
SHORT = {5: 3}          # frames cut to this many detections: frame 5 is below min_detections and keeps its planted outlier


@functools.lru_cache(maxsize=None)
def stream(distorted=False):
    """the contaminated recording: [(cam, mk, uv, bad)] per frame (raw corners when distorted)"""
    c = ld.case(distorted)
    out = []
    for f, (cam, mk, uv) in enumerate(c.frames):
        k = SHORT.get(f, len(cam))
        out.append(plant(cam[:k], mk[:k], uv[:k], PLAN[f]))
    return out


TIMES = [0.04 * f + 0.01 * (f % 3) for f in range(ld.FRAMES + 1)]          # uneven steps
