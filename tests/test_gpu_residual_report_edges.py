"""aar_problem_residual_report on crafted error distributions and shapes: every case of
tests/residual_report_cases.py on one GPU against the numpy restatement of tests/residual_report_restated.py fed with the device's own
per-detection errors -- median, max, threshold, keep flags and every count exactly, the sums to rounding --, the depth at which the
radix select resolves asserted from the device's bits, state left between calls, and the same sets sharded over 2 and 3 in-process ranks."""
import functools
import math
import threading

import numpy as np
import pytest

import aar
import residual_report_cases as rc
import residual_report_restated as rs
from aar import Problem

pytestmark = pytest.mark.gpu

ALL = rc.all_cases()
BY_NAME = {c.name: c for c in ALL}
SELECT = rc.select_cases()
RANK_CASES = rc.rank_cases()
RANK_BY_NAME = {c.name: c for c, _ in RANK_CASES}
ALL += [c for c, _ in RANK_CASES if c.name not in BY_NAME]      # (the sets built for the ranks alone are certified on one GPU as well)
COUNTS = ("num_detections", "num_rejected", "num_nonfinite", "cams_emptied", "markers_emptied", "frames_emptied")


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _resolve(rule, median, e):
    """the rule with the markers of residual_report_cases replaced by the device's own median / e_d[i], bit for bit"""
    if rule is None:
        return None
    k, m = rule
    if m == "median":
        m = median
    elif isinstance(m, str):
        m = e[int(m.split(":")[1])]
    return float(k), float(m)


def _report(p, x, rule):
    return p.residual_report(x, rule=False) if rule is None else p.residual_report(x, rule[0], rule[1], rule=True)


@functools.lru_cache(maxsize=None)
def _one_gpu(name):
    """one Problem per case: (e_d and sum r^2 from eval_residuals, [(rule, report)] for the case's rules); shared by the tests, never changed"""
    case = RANK_BY_NAME[name] if name in RANK_BY_NAME else BY_NAME[name]
    ds = case.ds
    with Problem(ds, residual_mode=case.mode) as p:
        r, _ = p.eval_residuals(case.x)
        r = r.reshape(-1, 8)
        ss = (r ** 2).sum(1)
        with np.errstate(invalid="ignore"):
            e_ref = np.sqrt(ss / 4)
        first = _report(p, case.x, None)
        runs = []
        for rule in case.rules:
            rule = _resolve(rule, first.report["median"], first.det_err)
            runs.append((rule, _report(p, case.x, rule)))
    return e_ref, ss, runs


def _certify(case, rr, e_ref, ss, rule):
    ds = case.ds
    np.testing.assert_allclose(rr.det_err, e_ref, rtol=1e-15, atol=0)
    want = rs.report(rr.det_err, ss, ds.obs_frame, ds.obs_cam, ds.obs_marker, ds.num_cams, ds.num_markers, ds.num_frames, rule)
    rep = rr.report
    for k in ("median", "max", "threshold"):
        assert _same(rep[k], want[k]), (case.name, rule, k, rep[k], want[k])
    assert np.array_equal(rr.keep, want["keep"]), (case.name, rule)
    for k in COUNTS:
        assert rep[k] == want[k], (case.name, rule, k, rep[k], want[k])
    for k in ("cam_stats", "marker_stats", "frame_stats"):
        np.testing.assert_array_equal(getattr(rr, k)[:, [0, 2, 3]], want[k][:, [0, 2, 3]], err_msg="%s %s %s" % (case.name, rule, k))
        np.testing.assert_allclose(getattr(rr, k)[:, 1], want[k][:, 1], rtol=1e-13, atol=0, err_msg="%s %s %s" % (case.name, rule, k))
    np.testing.assert_allclose(rep["sum_sq"], want["sum_sq"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(rep["rmse"], want["rmse"], rtol=1e-13, atol=0)
    return want


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_case_against_the_restatement(case):
    e_ref, ss, runs = _one_gpu(case.name)
    for rule, rr in runs:
        want = _certify(case, rr, e_ref, ss, rule)
        print("%s rule %s: median %r threshold %r, %d of %d rejected, emptied %d/%d/%d" % (
            case.name, rule, want["median"], want["threshold"], want["num_rejected"], want["num_detections"], want["cams_emptied"],
            want["markers_emptied"], want["frames_emptied"]))
        assert np.array_equal(rr.det_err, runs[0][1].det_err, equal_nan=True)     # the errors do not depend on the rule
    # what the builder promised holds on the device's bits as well
    e, cl = runs[0][1].det_err, case.claim
    if "tie_counts" in cl:
        _, counts = np.unique(rs.error_keys(e), return_counts=True)
        assert sorted(int(c) for c in counts if c > 1) == sorted(cl["tie_counts"])
    if "n_nan" in cl:
        assert int(np.isnan(e).sum()) == cl["n_nan"] and int(np.isposinf(e).sum()) == cl["n_inf"]
        assert math.isnan(runs[0][1].report["median"]) == cl["median_is_nan"]
    if "emptied" in cl:
        got = {rule: (rr.report["cams_emptied"], rr.report["markers_emptied"], rr.report["frames_emptied"]) for rule, rr in runs if rule is not None}
        for rule, counts in cl["emptied"].items():
            assert got[rule] == counts
    if "depth" in cl:
        assert rs.select_depth(e) == cl["depth"]


def test_threshold_on_an_error_value_keeps_exactly_the_values_up_to_it():
    """k_median = 1 and min_px = an e_d, bit for bit: the ties of that value stay, the next larger value goes"""
    seen = set()
    for case in ALL:
        for rule, rr in _one_gpu(case.name)[2]:
            if rule is None or not np.isfinite(rr.report["threshold"]):
                continue
            t, e = rr.report["threshold"], rr.det_err
            if (e == t).any():
                seen.add(case.name)
                assert rr.keep[e == t].all() and not rr.keep[e > t].any() and rr.keep[e < t].all()
    # every case carries such a rule (k_median = 1 at least), bar those whose median is NaN
    assert seen == set(c.name for c in ALL if not c.claim.get("median_is_nan"))


# ---------------------------------------------------------------- the depth at which the select resolves
@pytest.mark.parametrize("case", SELECT, ids=lambda c: c.name)
def test_select_resolves_at_the_depth_the_case_is_named_for(case):
    e = _one_gpu(case.name)[2][0][1].det_err
    k = np.sort(rs.error_keys(e)).astype(np.int64)
    depth = rs.select_depth(e)
    print("%s: depth %s on the device's bits, neighbouring keys %s ulp apart" % (case.name, depth, np.diff(k).tolist()))
    assert depth == case.claim["depth"]


def test_select_depths_cover_every_digit_and_the_tied_median():
    seen = {}
    for case in SELECT:
        seen.setdefault(rs.select_depth(_one_gpu(case.name)[2][0][1].det_err), []).append(case.name)
    print("one GPU:", seen)
    assert set(seen) == set(rc.DEPTHS)


# ---------------------------------------------------------------- nothing is left behind between calls
def test_state_between_calls():
    """one Problem, alternately a vector that resolves through the fetched single key at the second digit and one whose errors are all
    equal (six digits, no fetch): each call gives the bits of a fresh Problem"""
    case = rc.select_case(2, True)
    ds = case.ds
    xa = case.x
    xb = xa.copy()
    n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    xb[n0:] = np.tile(rc.POSE0, ds.num_frames)
    fresh = []
    for x in (xa, xb):
        with Problem(ds, residual_mode=case.mode) as p:
            fresh.append(p.residual_report(x, 1.0, 0.0))
    assert rs.select_depth(fresh[0].det_err) == 2 and rs.select_depth(fresh[1].det_err) == "all"
    assert len(set(fresh[1].det_err.tolist())) == 1 and fresh[0].report["median"] != fresh[1].report["median"]
    with Problem(ds, residual_mode=case.mode) as p:
        for i in range(6):
            rr, want = p.residual_report((xa, xb)[i % 2], 1.0, 0.0), fresh[i % 2]
            for k in ("det_err", "keep", "cam_stats", "marker_stats", "frame_stats"):
                assert np.array_equal(getattr(rr, k), getattr(want, k)), (i, k)
            assert rr.report == want.report, i


# ---------------------------------------------------------------- sharded over in-process ranks
@functools.lru_cache(maxsize=None)
def _ranks(world, name):
    case = RANK_BY_NAME[name]
    one = _one_gpu(name)[2]
    rules = [rule for rule, _ in one]
    group = aar.LocalGroup(world)
    out = [None] * world

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with Problem(case.ds, comm=comm, residual_mode=case.mode) as p:
                out[r] = [_report(p, case.x, rule) for rule in rules]
        except Exception as e:
            out[r] = e
        finally:
            comm.close()
    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    group.close()
    for o in out:
        assert not isinstance(o, Exception), o
    return out


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", [c.name for c, _ in RANK_CASES])
def test_ranks_agree_with_one_gpu(world, name):
    case = RANK_BY_NAME[name]
    ds = case.ds
    begin = aar.plan_shards(np.bincount(ds.obs_frame, minlength=ds.num_frames), world)
    out = _ranks(world, name)
    for i, (rule, one) in enumerate(_one_gpu(name)[2]):
        got = [o[i] for o in out]
        assert np.array_equal(np.concatenate([g.keep for g in got]), one.keep)
        assert np.array_equal(np.concatenate([g.det_err for g in got]), one.det_err, equal_nan=True)
        for r, g in enumerate(got):
            for k in ("median", "max", "threshold") + COUNTS:
                assert _same(g.report[k], one.report[k]), (name, world, rule, r, k, g.report[k], one.report[k])
            np.testing.assert_allclose(g.report["sum_sq"], one.report["sum_sq"], rtol=1e-12, atol=0)
            for k in ("cam_stats", "marker_stats"):
                assert np.array_equal(getattr(g, k), getattr(got[0], k), equal_nan=True)          # the same bits on every rank
                np.testing.assert_array_equal(getattr(g, k)[:, [0, 2, 3]], getattr(one, k)[:, [0, 2, 3]])
                np.testing.assert_allclose(getattr(g, k)[:, 1], getattr(one, k)[:, 1], rtol=1e-12, atol=0)
            mine = slice(int(begin[r]), int(begin[r + 1]))
            assert len(g.det_err) == int((np.asarray(ds.obs_frame) >= begin[r]).sum() - (np.asarray(ds.obs_frame) >= begin[r + 1]).sum())
            assert np.array_equal(g.frame_stats[mine], one.frame_stats[mine], equal_nan=True)
    if name == "one_frame" and world == 2:
        assert sorted(len(o[0].det_err) for o in out) == [0, ds.num_obs]       # one rank has no frames


@pytest.mark.parametrize("world", [2, 3])
def test_select_depths_are_covered_on_ranks(world):
    seen = {}
    for case, why in RANK_CASES:
        if why == "depth":
            e = np.concatenate([o[0].det_err for o in _ranks(world, case.name)])
            depth = rs.select_depth(e)
            assert depth == case.claim["depth"]
            seen[depth] = case.name
    print("world %d:" % world, seen)
    assert set(seen) == set(rc.DEPTHS)
