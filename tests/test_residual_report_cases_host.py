"""The residual-report certificate without a GPU: the numpy restatement against brute-force definitions on random
arrays with injected ties, NaN and +inf, and every case builder against what it claims -- tie counts, ladder depths, frame and run sizes,
emptied entities -- under the float64 projection of projection_reference.  CPU only."""
import math
import struct

import numpy as np
import pytest

import residual_report_cases as rc
import residual_report_restated as rs

ALL = rc.all_cases()


# ---------------------------------------------------------------- brute force: python integers and explicit loops
def _key(v):
    return 0x7FF8000000000000 if math.isnan(v) else struct.unpack("<Q", struct.pack("<d", abs(v)))[0]


def _value(k):
    return struct.unpack("<d", struct.pack("<Q", k))[0]


def _brute(e, ss, of, oc, om, C, M, F, rule):
    n = len(e)
    keys = np.sort(np.array([_key(float(v)) for v in e], dtype=np.uint64))
    med = _value(int(keys[(n - 1) // 2]))
    mx = float("nan") if any(math.isnan(v) for v in e) else _value(int(keys[-1]))
    if rule is None or (rule[0] <= 0 and rule[1] <= 0):
        t = float("inf")
    elif rule[0] <= 0:
        t = rule[1]
    else:
        a = rule[0] * med
        t = a if a > rule[1] else rule[1]
    keep = [bool(v <= t) for v in e]
    tabs = []
    for idx, cnt in ((oc, C), (om, M), (of, F)):
        tab = np.zeros((cnt, 4))
        for i in range(cnt):
            mine = [o for o in range(n) if idx[o] == i]
            if not mine:
                continue
            top = max(_key(float(e[o])) for o in mine)
            tab[i] = (len(mine), sum(float(ss[o]) for o in mine), _value(top), sum(1 for o in mine if not keep[o]))
        tabs.append(tab)
    emptied = [sum(1 for row in tab if row[0] > 0 and row[3] == row[0]) for tab in tabs]
    return dict(median=med, max=mx, threshold=t, keep=np.array(keep), num_rejected=keep.count(False),
                num_nonfinite=sum(1 for v in e if not math.isfinite(v)), cam_stats=tabs[0], marker_stats=tabs[1], frame_stats=tabs[2],
                cams_emptied=emptied[0], markers_emptied=emptied[1], frames_emptied=emptied[2])


def _brute_depth(e):
    keys = sorted(_key(float(v)) for v in e)
    mk = keys[(len(keys) - 1) // 2]
    for digit, low in enumerate((52, 41, 30, 19, 8, 0), start=1):
        if sum(1 for k in keys if k >> low == mk >> low) == 1:
            return digit
    return "all"


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _random_errors(rng, n, n_nan, n_inf, ties):
    e = rng.uniform(0.1, 3.0, n) * 2.0 ** rng.integers(-3, 4, n)
    if ties and n > 1:
        src = rng.integers(0, n, n // 2)
        e[rng.integers(0, n, n // 2)] = e[src]
    where = rng.permutation(n)
    e[where[:n_nan]] = np.nan
    e[where[n_nan:n_nan + n_inf]] = np.inf
    return e


@pytest.mark.parametrize("seed", range(12))
def test_restatement_against_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    n = [1, 2, 3, 4, 7, 16, 61, 120, 200, 33, 50, 9][seed]
    n_nan = [0, 0, 1, 0, 2, 0, 31, 0, 150, 17, 0, 9][seed]
    n_inf = [0, 1, 0, 0, 1, 3, 0, 60, 10, 0, 0, 0][seed]
    C, M, F = 4, 5, 7
    e = _random_errors(rng, n, n_nan, min(n_inf, n - n_nan), ties=seed % 2 == 0)
    ss = 4 * e * e
    of, oc, om = np.sort(rng.integers(0, F, n)), rng.integers(0, C - 1, n), rng.integers(1, M, n)   # camera C-1 and marker 0: no detections
    finite = e[np.isfinite(e)]
    some = float(finite[0]) if len(finite) else 1.0
    for rule in (None, (0.0, 0.0), (1.0, 0.0), (3.0, 0.0), (0.0, some), (0.5, some), (4.0, some), (-1.0, some), (1.0, np.inf), (0.0, 1e-9)):
        got = rs.report(e, ss, of, oc, om, C, M, F, rule)
        want = _brute(e, ss, of, oc, om, C, M, F, rule)
        for k in ("median", "max", "threshold"):
            assert _same(got[k], want[k]), (rule, k, got[k], want[k])
        assert np.array_equal(got["keep"], want["keep"]), rule
        for k in ("num_rejected", "num_nonfinite", "cams_emptied", "markers_emptied", "frames_emptied"):
            assert got[k] == want[k], (rule, k)
        assert got["num_detections"] == n
        for k in ("cam_stats", "marker_stats", "frame_stats"):
            np.testing.assert_array_equal(got[k][:, [0, 2, 3]], want[k][:, [0, 2, 3]], err_msg=k)
            np.testing.assert_allclose(got[k][:, 1], want[k][:, 1], rtol=1e-13, atol=0, err_msg=k)
        with np.errstate(invalid="ignore"):
            np.testing.assert_allclose(got["sum_sq"], ss.sum(), rtol=1e-13)
            np.testing.assert_allclose(got["rmse"], np.sqrt(ss.sum() / (4 * n)), rtol=1e-13)
    assert rs.select_depth(e) == _brute_depth(e)
    # the median of a NaN majority is NaN, and a rule on it falls back to min_px: k * NaN > min_px is false
    if n_nan >= n - (n - 1) // 2:
        assert math.isnan(rs.lower_median(e)) and rs.threshold(True, 3.0, 0.25, float("nan")) == 0.25


def test_restatement_select_depth_on_written_keys():
    """keys written bit by bit: alone at each digit in turn, and never"""
    base = 0x4061A00000000000
    for digit, low in enumerate(rs.DIGIT_BOUNDS, start=1):
        keys = np.array([base, base + (1 << low), base + (2 << low)], dtype=np.uint64)
        if digit > 1:       # ... and a pair that shares the median's bucket one digit earlier is what keeps it from resolving there
            assert rs.select_depth(keys.view(np.float64)) == digit == _brute_depth(keys.view(np.float64))
        else:
            assert rs.select_depth(keys.view(np.float64)) == 1
    keys = np.array([base, base + 1, base + 1, base + 2], dtype=np.uint64)
    assert rs.select_depth(keys.view(np.float64)) == "all"
    assert rs.select_depth(np.array([1.0, np.nan, np.nan])) == "all"
    assert rs.select_depth(np.array([1.0, np.inf, np.nan])) == 2      # +inf and NaN share the exponent digit and part in the next one
    assert rs.select_depth(np.array([3.5])) == 1


# ---------------------------------------------------------------- the builders against their claims
def _tie_sizes(e):
    _, counts = np.unique(rs.error_keys(e), return_counts=True)
    return sorted(int(c) for c in counts if c > 1)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_case_is_what_it_claims(case):
    ds, cl = case.ds, case.claim
    e, ss = rc.host_errors(case)
    n = ds.num_obs
    assert ds.num_cams <= 6 and ds.num_markers <= 26 and ds.num_frames <= 130 and 0 < n <= 460 and len(e) == n
    assert (np.diff(ds.obs_frame) >= 0).all()
    if "depth" in cl:
        assert rs.select_depth(e) == cl["depth"]
    if "tie_counts" in cl:
        assert _tie_sizes(e) == sorted(cl["tie_counts"])
    if "n" in cl:
        assert n == cl["n"] and len(set(e.tolist())) == n
        if n == 4:
            s = np.sort(e)
            assert s[1] < s[2] and rs.lower_median(e) == s[1]
    if "n_nan" in cl:
        assert int(np.isnan(e).sum()) == cl["n_nan"] and int(np.isposinf(e).sum()) == cl["n_inf"]
        assert math.isnan(rs.lower_median(e)) == cl["median_is_nan"]
    if "frame_sizes" in cl:
        assert np.bincount(ds.obs_frame, minlength=ds.num_frames).tolist() == cl["frame_sizes"]
    if "run_lengths" in cl:
        _, counts = np.unique(np.asarray(ds.obs_cam) * ds.num_markers + np.asarray(ds.obs_marker), return_counts=True)
        assert sorted(counts.tolist()) == sorted(cl["run_lengths"])
        assert (np.bincount(ds.obs_cam, minlength=ds.num_cams) == 0).any() and (np.bincount(ds.obs_marker, minlength=ds.num_markers) == 0).any()
    if "emptied" in cl:
        assert (np.bincount(ds.obs_cam, minlength=ds.num_cams) == 0).any() and (np.bincount(ds.obs_marker, minlength=ds.num_markers) == 0).any()
        for rule, (cams, mks, frs) in cl["emptied"].items():
            r = rs.report(e, ss, ds.obs_frame, ds.obs_cam, ds.obs_marker, ds.num_cams, ds.num_markers, ds.num_frames, rule)
            assert (r["cams_emptied"], r["markers_emptied"], r["frames_emptied"]) == (cams, mks, frs)
            assert len({cams, mks, frs}) == 3 and min(cams, mks, frs) > 0
    if "low_frames" in cl:     # the two-value sets: where the median sits relative to the block of low values
        k_low, rank = len(cl["low_frames"]), (n - 1) // 2
        lo, hi = np.unique(e)
        assert rs.lower_median(e) == (lo if rank < k_low else hi)
        assert (e[np.isin(ds.obs_frame, cl["low_frames"])] == lo).all()


def test_two_value_sets_put_the_rank_on_both_sides_of_the_boundary():
    seen = set()
    for c in ALL:
        if "low_frames" in c.claim:
            seen.add(len(c.claim["low_frames"]) - (c.ds.num_obs - 1) // 2)
    assert seen == {0, 1, 2}


def test_ladder_exponents_sit_inside_their_digits():
    """one step of the ladder, in ulp, lies in [2 x 2^low, 2^(low + 11) / 16] of its digit (bits [low, low + 11)): neighbours never share a bucket
    of that digit, and the whole ladder spans at most half a bucket of the digit above, so the median shares that one with a neighbour"""
    for depth, m in rc.LADDER_M.items():
        case = rc.select_case(depth, True)
        k = np.sort(rs.error_keys(rc.host_errors(case)[0])).astype(np.int64)
        step = np.diff(k)
        low = rs.DIGIT_BOUNDS[depth - 1]
        assert (step > 0).all()
        print("depth %d, m = %d: steps of %d .. %d ulp" % (depth, m, step.min(), step.max()))
        if depth < 6:
            assert step.min() >= 2 * 2 ** low and step.max() <= 2 ** (low + 11) // 16
        else:
            assert 4 <= step.min() and step.max() <= 16


def test_select_cases_cover_every_depth():
    seen = {}
    for c in rc.select_cases():
        seen.setdefault(rs.select_depth(rc.host_errors(c)[0]), []).append(c.ds.num_obs % 2)
    assert set(seen) == set(rc.DEPTHS)
    assert all(sorted(set(v)) == [0, 1] for v in seen.values())     # each at an odd and an even N


def test_rank_cases_are_where_they_should_be():
    import aar
    for case, why in rc.rank_cases():
        per_frame = np.bincount(case.ds.obs_frame, minlength=case.ds.num_frames)
        e, _ = rc.host_errors(case)
        for world in (2, 3):
            begin = aar.plan_shards(per_frame, world)
            if why == "split_ties":        # the largest block of equal values has members on both sides of a boundary
                keys = rs.error_keys(e)
                vals, counts = np.unique(keys, return_counts=True)
                frames = np.asarray(case.ds.obs_frame)[keys == vals[np.argmax(counts)]]
                owner = np.searchsorted(np.asarray(begin)[1:], frames, side="right")
                assert len(set(owner.tolist())) >= 2, (case.name, world)
            if why == "last_rank":
                f = case.claim["median_frame"]
                assert e[np.asarray(case.ds.obs_frame) == f][0] == rs.lower_median(e) and begin[world - 1] <= f
            if why == "one_frame" and world == 2:
                assert case.ds.num_frames == 1 and (begin[1] - begin[0] == 0 or begin[2] - begin[1] == 0)
