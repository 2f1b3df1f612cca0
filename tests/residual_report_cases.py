"""Crafted data sets for the residual-report certificate.

TEST INFRASTRUCTURE ONLY (numpy): imported by tests/test_residual_report_cases_host.py and tests/test_gpu_residual_report_edges.py.

Every data set is built by projection_reference.build_dataset at given poses with noise_px = 0; then obs_uv / x_full are overwritten.  Two
techniques give exact structure without assuming anything about the device's rounding:

  ties     In a scene every non-root camera carries ONE 6-vector and one camera matrix, and so does every non-root marker.  Detections
           of (clone camera, clone marker) in frames with identical 6-vectors whose corners were shifted by the same amount are the
           same inputs through the same instructions: bit-identical e_d, whatever the instructions are.
  ladders  N frames hold one detection each of the same pair, corners shifted by +100 px; frame k is evaluated with t_z scaled by
           1 + k 2^-m.  The keys share their leading digits and part at a depth set by m (measured with the float64 projection, and
           asserted again from the device's own bits by the GPU test):  m = 6 -> 2, 17 -> 3, 28 -> 4, 38 -> 5, 45 -> 6.  The pair is
           (root camera, root marker), where one step of k moves e_d by about 2^(48.4 - m) ulp: at these exponents a step is at least
           twice the weight of its digit's lowest bit -- two neighbours never share that digit's bucket -- and at most 1/16 of the
           bucket above, which the median therefore shares with a neighbour; a few ulp of difference between two evaluations of the
           projection cannot change either.  m = 48 (a quarter of an ulp per step) collapses into ties.

Non-finite errors: a NaN frame pose gives NaN for every detection of the frame.  A +inf corner in obs_uv (problem creation does not look
at the corners' values) gives r = +inf in both residual modes, hence e_d = +inf without a NaN.

A case is (name, ds, x, mode, rules, claim).  `x` is the evaluation point, `rules` a list of None (no rule) or (k_median, min_px); the
marker "median" / "value:<i>" in place of min_px stands for "the device's own median / e_d[i], bit for bit" and is resolved by the test
that runs the case.  `claim` holds what the builder promises: the host test checks it under the float64 projection.
"""
import numpy as np

import projection_reference as pr
from projection_reference import RES_F32, RES_F64

SHIFT = 100.0


class Case:
    def __init__(self, name, ds, x, mode=RES_F64, rules=(None,), **claim):
        self.name, self.ds, self.x, self.mode, self.rules, self.claim = name, ds, np.asarray(x, dtype=np.float64), mode, list(rules), claim

    def __repr__(self):
        return self.name


def host_errors(case):
    """(e_d, sum r^2 per detection) under the float64 projection of projection_reference, in the case's residual mode"""
    with np.errstate(all="ignore"):
        r = pr.Reference(case.ds).residuals(case.x, case.mode).reshape(-1, 8)
        ss = (r ** 2).sum(1)
        return np.sqrt(ss / 4), ss


# ---------------------------------------------------------------- the clone scene
CLONE_CAM = pr.camera_looking_at_centre(pr.rotvec([0.3, 1.0, 0.1], 0.4), np.array([0.05, -0.02, 0.03]))
CLONE_MARKER = np.concatenate([pr.rotvec([1.0, -0.5, 0.2], 0.2), [0.06, -0.04, 0.01]])
POSE0 = np.concatenate([pr.rotvec([0.2, 0.5, -1.0], 0.3), pr.OBJECT_CENTRE + [0.02, 0.03, -0.05]])


def pose(i):
    """a distinct, well-conditioned frame pose per integer i (pose(0) = POSE0)"""
    p = POSE0.copy()
    p[:3] += 0.01 * np.array([np.sin(1.3 * i), np.cos(2.1 * i) - 1, np.sin(0.7 * i)])
    p[3:] += 0.02 * np.array([np.sin(0.9 * i), np.sin(1.7 * i), np.cos(1.1 * i) - 1])
    return p


class Scene:
    """Frames are added one by one: (6-vector the corners are generated at, 6-vector of the evaluation point, detections).  A detection is
    (camera, marker, shift in px added to all eight coordinates in float)."""

    def __init__(self, C=2, M=2):
        self.C, self.M = C, M
        self.frames = []

    def frame(self, dets, base=None, at=None):
        base = POSE0 if base is None else np.asarray(base, dtype=np.float64)
        self.frames.append((base, base if at is None else np.asarray(at, dtype=np.float64), sorted(dets)))
        return len(self.frames) - 1

    def build(self):
        C, M, F = self.C, self.M, len(self.frames)
        cams = np.tile(CLONE_CAM, (C, 1)); mks = np.tile(CLONE_MARKER, (M, 1))
        of, oc, om, shift = [], [], [], []
        for f, (_, _, dets) in enumerate(self.frames):
            for c, m, s in dets:
                of.append(f); oc.append(c); om.append(m); shift.append(s)
        ds = pr.build_dataset(cams, mks, np.array([b for b, _, _ in self.frames]).reshape(F, 6), of, oc, om, noise_px=0.0)
        uv = np.array(ds.obs_uv, dtype=np.float32).reshape(-1, 8)
        with np.errstate(all="ignore"):
            uv = (uv + np.asarray(shift, dtype=np.float32).reshape(-1, 1)).astype(np.float32)
        ds.obs_uv = uv.reshape(np.asarray(ds.obs_uv).shape)
        x = ds.x_full.copy()
        n0 = 6 * (C - 1) + 6 * (M - 1)
        x[n0:] = np.array([a for _, a, _ in self.frames]).reshape(-1)
        ds.x_full = x
        return ds, x


def scaled_tz(k, m):
    p = POSE0.copy()
    p[5] = POSE0[5] * (1.0 + k * 2.0 ** -m)
    return p


def add_ladder(sc, ks, m, shift=SHIFT, pair=(0, 0)):
    return [sc.frame([(pair[0], pair[1], shift)], at=scaled_tz(k, m)) for k in ks]


def add_ties(sc, n, shift, pair=(1, 1), per_frame=1, base=None):
    """n bit-identical detections: per_frame of them in each frame (clone pairs (c, m), c and m from pair upwards), identical frame poses"""
    pairs = [(c, m) for c in range(pair[0], sc.C) for m in range(pair[1], sc.M)][:per_frame]
    assert len(pairs) == per_frame
    out = []
    while n > 0:
        take = min(n, per_frame)
        out.append(sc.frame([(c, m, shift) for c, m in pairs[:take]], base=base))
        n -= take
    return out


# ---------------------------------------------------------------- select depth
LADDER_M = {2: 6, 3: 17, 4: 28, 5: 38, 6: 45}
DEPTHS = (1, 2, 3, 4, 5, 6, "all")
LADDER_RULES = [None, (1.0, 0.0), (3.0, 0.0), (0.0, "median"), (0.5, "value:0"), (1.0, 1e4), (0.0, 0.0)]


def select_case(depth, n_even):
    """a case whose select resolves at `depth`; N = 5 (odd) or 8 (even), depth 1: 3 or 4"""
    sc = Scene()
    if depth == 1:        # different binary exponents: every key is alone after the first digit
        for s in (1.0, 100.0, 10000.0, 1.0e6)[:4 if n_even else 3]:
            sc.frame([(1, 1, s)])
    elif depth == "all":  # a depth-3 ladder whose median step is there twice: the median is a tied value, no bucket on its way holds one key
        add_ladder(sc, [0, 1, 2, 3, 3, 4, 5, 6] if n_even else [0, 1, 2, 2, 3], LADDER_M[3])
    else:
        add_ladder(sc, range(8 if n_even else 5), LADDER_M[depth])
    ds, x = sc.build()
    return Case("select_%s_%s" % (depth, "even" if n_even else "odd"), ds, x, rules=LADDER_RULES, depth=depth)


def select_cases():
    return [select_case(d, ev) for d in DEPTHS for ev in (False, True)]


def collapse_cases():
    """ladders whose steps are below the resolution: m = 48 in float64 residuals, and the depth-5 / depth-6 ladders in RES_F32, where the
    projection is rounded to float before the subtraction.  No depth is promised: whatever ties the rounding makes, the report is exact."""
    out = []
    for name, m, mode in (("collapse_m48", 48, RES_F64), ("collapse_f32_m38", 38, RES_F32), ("collapse_f32_m45", 45, RES_F32)):
        for n in (5, 8):
            sc = Scene()
            add_ladder(sc, range(n), m)
            ds, x = sc.build()
            out.append(Case("%s_n%d" % (name, n), ds, x, mode=mode, rules=[None, (1.0, 0.0), (0.0, "median")]))
    return out


# ---------------------------------------------------------------- small N
def small_n_cases():
    out = []
    for n in (1, 2, 3, 4):
        sc = Scene()
        for i in range(n):     # distinct values of one magnitude: N = 4 has two distinct middle values, the lower one is the median
            sc.frame([(1, 1, SHIFT + 7.0 * ((3 * i) % 4))])
        ds, x = sc.build()
        out.append(Case("small_n%d" % n, ds, x, rules=[None, (1.0, 0.0), (2.0, 0.0), (0.0, "median"), (0.0, 0.0)], n=n))
    return out


# ---------------------------------------------------------------- tied values
TIE_RULES = [None, (1.0, 0.0), (0.0, "median"), (0.0, "value:0"), (0.5, "median"), (2.0, "median"), (0.0, 0.0), (1.0, 1e4)]


def all_equal_case(n):
    sc = Scene(5, 26) if n > 130 else Scene()
    add_ties(sc, n, SHIFT, per_frame=100 if n > 130 else 1)
    ds, x = sc.build()
    return Case("all_equal_n%d" % n, ds, x, rules=TIE_RULES, tie_counts=[n])


def two_value_case(n, k_low):
    """k_low copies of the lower value, n - k_low of the higher (same magnitude: they part at the second digit)"""
    sc = Scene()
    hi = add_ties(sc, (n - k_low + 1) // 2, SHIFT + 20.0)          # interleaved in frame order: high, low, high
    lo = add_ties(sc, k_low, SHIFT)
    hi += add_ties(sc, (n - k_low) // 2, SHIFT + 20.0)
    ds, x = sc.build()
    return Case("two_values_n%d_low%d" % (n, k_low), ds, x, rules=TIE_RULES, tie_counts=[k_low, n - k_low], low_frames=lo, high_frames=hi)


def tie_cases():
    out = [all_equal_case(n) for n in (2, 7, 300)]
    for n in (9, 10):
        rank = (n - 1) // 2
        out += [two_value_case(n, k) for k in (rank, rank + 1, rank + 2)]   # the median is the higher value, the last low one, a low one
    return out


def mixed_cases():
    """a tied block that holds the median with a ladder of larger values behind it, and a ladder that holds the median between tied blocks"""
    out = []
    for m in (17, 45):
        sc = Scene()
        add_ties(sc, 6, 50.0)
        add_ladder(sc, range(5), m)                                     # n = 11, rank 5: the last of the six tied values
        ds, x = sc.build()
        out.append(Case("ties_then_ladder_m%d" % m, ds, x, rules=TIE_RULES, tie_counts=[6], depth="all"))
        sc = Scene()
        add_ties(sc, 3, 50.0)
        add_ladder(sc, range(5), m)
        add_ties(sc, 4, 400.0)                                          # n = 12, rank 5: the ladder's middle step
        ds, x = sc.build()
        out.append(Case("ladder_between_ties_m%d" % m, ds, x, rules=TIE_RULES, tie_counts=[3, 4], depth={17: 3, 45: 6}[m]))
    return out


# ---------------------------------------------------------------- non-finite errors
def _nan_frame(x, C, M, f):
    x = x.copy()
    n0 = 6 * (C - 1) + 6 * (M - 1)
    x[n0 + 6 * f:n0 + 6 * f + 6] = np.nan
    return x


NONFINITE_RULES = [None, (3.0, 0.0), (1.0, 0.0), (2.0, 150.0), (0.0, 150.0), (0.0, 0.0)]


def nonfinite_cases():
    out = []
    n = 9                                   # rank 4
    for j, tag in ((2, "few"), (4, "rank"), (5, "rank_plus_1"), (9, "all")):
        sc = Scene(3, 4)
        pairs = [(c, m) for c in range(3) for m in range(4)]
        bad = sc.frame([(c, m, SHIFT) for c, m in pairs[:j]], base=pose(1))
        for i in range(n - j):
            sc.frame([(1, 1, SHIFT + 5.0 * i)], base=pose(2 + i))
        ds, x = sc.build()
        out.append(Case("nan_frame_%s" % tag, ds, _nan_frame(x, 3, 4, bad), rules=NONFINITE_RULES, n_nan=j, n_inf=0, median_is_nan=j >= n - 4))
    for with_nan in (False, True):
        sc = Scene(3, 4)
        sc.frame([(1, 1, SHIFT), (1, 2, SHIFT), (2, 1, SHIFT)], base=pose(1))
        for i in range(4):
            sc.frame([(0, 0, SHIFT + 5.0 * i), (1, 1, SHIFT + 3.0 * i)], base=pose(2 + i))
        ds, x = sc.build()
        uv = np.array(ds.obs_uv, dtype=np.float32).reshape(-1, 8)
        uv[4, 3] = np.inf                   # one coordinate of one corner of a detection of frame 1
        ds.obs_uv = uv.reshape(np.asarray(ds.obs_uv).shape)
        if with_nan:
            x = _nan_frame(x, 3, 4, 0)
        out.append(Case("inf_corner_with_nan" if with_nan else "inf_corner", ds, x, rules=NONFINITE_RULES + [(0.0, np.inf), (1.0, np.inf)],
                        n_nan=3 if with_nan else 0, n_inf=1, median_is_nan=False))
    return out


# ---------------------------------------------------------------- shapes
FRAME_SIZES = {1: [129], 2: [64, 0], 3: [65, 1, 63], 4: [128, 2, 0, 64], 5: [63, 129, 0, 65, 1], 9: [0, 1, 2, 63, 64, 65, 128, 129, 0]}
RUN_LENGTHS = [1, 64, 65, 130]
SHAPE_RULES = [None, (1.0, 0.0), (1.5, 0.0), (0.0, "median"), (0.0, "value:0")]


def shape_cases():
    out = []
    for F, sizes in FRAME_SIZES.items():
        ds = pr.frame_counts_dataset(sizes, C=5, M=26, seed=40 + F)
        out.append(Case("frame_sizes_F%d" % F, ds, ds.x_full, rules=SHAPE_RULES, frame_sizes=sizes))
    ds = pr.run_lengths_dataset(RUN_LENGTHS, C=5, M=6, seed=61)
    out.append(Case("run_lengths", ds, ds.x_full, rules=SHAPE_RULES, run_lengths=RUN_LENGTHS, unobserved=True))
    return out


# ---------------------------------------------------------------- a rule that empties entities
def emptied_case():
    """frames 0-5: cameras 0-2 x markers 0-4, small errors.  Frames 6-8: cameras 3 and 4 see marker 5 and nothing else, large errors.
    A rule between the two empties 3 frames, 2 cameras and 1 marker; camera 5 and marker 6 have no detections and are not counted."""
    sc = Scene(6, 7)
    for f in range(6):
        sc.frame([(c, m, 10.0 + f) for c in range(3) for m in range(5)], base=pose(f))
    for f in range(3):
        sc.frame([(3, 5, 500.0), (4, 5, 500.0 + f)], base=pose(10 + f))
    ds, x = sc.build()
    return Case("emptied", ds, x, rules=[None, (3.0, 0.0), (0.0, 100.0), (1.0, 0.0), (0.0, 1e-3), (0.0, 0.0)],
                emptied={(3.0, 0.0): (2, 1, 3), (0.0, 100.0): (2, 1, 3), (0.0, 1e-3): (5, 6, 9)})


def all_cases():
    return select_cases() + collapse_cases() + small_n_cases() + tie_cases() + mixed_cases() + nonfinite_cases() + shape_cases() + [emptied_case()]


# ---------------------------------------------------------------- sharded runs
def rank_cases():
    """(case, what it is there for): the select cases with even N (every depth), tied blocks that straddle the shard boundaries, a set whose
    median lies on the last rank, one frame (a rank without frames at world 2)"""
    out = [(select_case(d, True), "depth") for d in DEPTHS]
    out += [(all_equal_case(7), "split_ties"), (two_value_case(10, 5), "split_ties"), (mixed_cases()[0], "split_ties")]
    sc = Scene()
    for s in (10.0, 20.0, 30.0, 50.0, 60.0, 70.0, 40.0, 80.0):     # rank 3 of 8: the value 40 in frame 6, on the last rank of 2 and of 3
        sc.frame([(1, 1, s)])
    ds, x = sc.build()
    out.append((Case("median_on_last_rank", ds, x, rules=[(1.0, 0.0)], median_frame=6), "last_rank"))
    sc = Scene(3, 4)
    sc.frame([(c, m, SHIFT + 3.0 * c + m) for c in range(3) for m in range(4)])
    ds, x = sc.build()
    out.append((Case("one_frame", ds, x, rules=[(1.0, 0.0)]), "one_frame"))
    return out
