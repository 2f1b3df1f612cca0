"""aar_problem_residual_report restated in numpy (DESIGN.md sections 14 and 27).

TEST INFRASTRUCTURE ONLY: imported by tests/residual_report_cases.py, tests/test_residual_report_cases_host.py and
tests/test_gpu_residual_report_edges.py.  It shares nothing with `_check_rule` / `_groupby` of tests/test_gpu_residual_report.py: the order
is the order of the 63-bit integer keys, and every table comes from integer counting (bincount) and maximum.at on those keys.

    key(e)   the bits of |e|; a NaN maps to 0x7FF8000000000000, above +inf (0x7FF0000000000000)
    median   the value whose key is element (n - 1) // 2 of the ascending keys (the LOWER median)
    max      the value of the largest key; NaN if any e is NaN
    t        +inf without a rule or with k_median <= 0 and min_px <= 0; min_px with k_median <= 0; else a = k_median * median and
             `a if a > min_px else min_px`.  A NaN median (half or more of the detections NaN) therefore gives min_px: the comparison
             is false.  This is the BATCH rule; the live gate of section 24 treats a non-finite error as +inf and gives +inf there.
    keep     e <= t: a NaN is never kept, +inf only by t = +inf
    tables   per camera / marker / frame {detections, sum r^2, max, rejected}, zeros for an entity without detections
    emptied  entities with detections all of which are rejected
"""
import numpy as np

NAN_KEY = np.uint64(0x7FF8000000000000)
ABS_MASK = np.uint64(0x7FFFFFFFFFFFFFFF)
DIGIT_BOUNDS = (52, 41, 30, 19, 8, 0)      # the select's six digits: bits [52, 63), [41, 52), [30, 41), [19, 30), [8, 19), [0, 8)


def error_keys(e):
    e = np.ascontiguousarray(e, dtype=np.float64)
    k = e.view(np.uint64) & ABS_MASK
    return np.where(np.isnan(e), NAN_KEY, k)


def key_values(k):
    return np.ascontiguousarray(k, dtype=np.uint64).view(np.float64)


def lower_median(e):
    k = np.sort(error_keys(e))
    return float(key_values(k[(len(k) - 1) // 2:(len(k) - 1) // 2 + 1])[0]) if len(k) else float("nan")


def threshold(has_rule, k_median, min_px, median):
    if not has_rule or (k_median <= 0.0 and min_px <= 0.0):
        return float("inf")
    if k_median <= 0.0:
        return float(min_px)
    a = k_median * median
    return float(a) if a > min_px else float(min_px)


def _table(idx, n, keys, ss, rejected):
    idx = np.asarray(idx, dtype=np.int64)
    t = np.zeros((n, 4))
    t[:, 0] = np.bincount(idx, minlength=n)
    with np.errstate(invalid="ignore"):                       # (+inf and NaN may meet in one entity: the sum is NaN, as it must be)
        for i, s in zip(idx, ss):                             # plain ascending accumulation: to rounding only
            t[i, 1] += s
    top = np.zeros(n, dtype=np.uint64)
    np.maximum.at(top, idx, keys)
    t[:, 2] = key_values(top)
    t[:, 3] = np.bincount(idx, weights=rejected.astype(np.float64), minlength=n)
    return t


def report(det_err, sum_r2, obs_frame, obs_cam, obs_marker, C, M, F, rule=None):
    """Everything one call returns, from the per-detection errors and their sum r^2.  rule: None (no rule) or (k_median, min_px)."""
    e = np.ascontiguousarray(det_err, dtype=np.float64)
    ss = np.ascontiguousarray(sum_r2, dtype=np.float64)
    n = len(e)
    keys = error_keys(e)
    med = lower_median(e)
    n_nan = int(np.isnan(e).sum())
    mx = float("nan") if (n_nan or n == 0) else float(key_values(keys.max(keepdims=True))[0])
    has_rule = rule is not None
    t = threshold(has_rule, rule[0] if has_rule else 0.0, rule[1] if has_rule else 0.0, med)
    keep = np.zeros(n, dtype=bool)
    for i in range(n):
        keep[i] = (not np.isnan(e[i])) and e[i] <= t
    rej = ~keep
    cams = _table(obs_cam, C, keys, ss, rej)
    mks = _table(obs_marker, M, keys, ss, rej)
    frs = _table(obs_frame, F, keys, ss, rej)
    emptied = lambda tab: int(((tab[:, 0] > 0) & (tab[:, 3] == tab[:, 0])).sum())
    with np.errstate(invalid="ignore"):
        sum_sq = float(cams[:, 1].sum())
    return dict(median=med, max=mx, threshold=t, keep=keep, num_detections=n, num_rejected=int(rej.sum()),
                num_nonfinite=int((~np.isfinite(e)).sum()), cam_stats=cams, marker_stats=mks, frame_stats=frs,
                cams_emptied=emptied(cams), markers_emptied=emptied(mks), frames_emptied=emptied(frs),
                sum_sq=sum_sq, rmse=float(np.sqrt(sum_sq / (4.0 * n))) if n else float("nan"))


def select_depth(det_err):
    """The first digit 1 .. 6 at which the median's key is alone in its bucket (the device then fetches the key and stops), or "all" when
    it never is: the median is a tied value and all six digits are counted."""
    keys = error_keys(det_err)
    mk = np.sort(keys)[(len(keys) - 1) // 2]
    for digit, low in enumerate(DIGIT_BOUNDS, start=1):
        if int(((keys >> np.uint64(low)) == (mk >> np.uint64(low))).sum()) == 1:
            return digit
    return "all"
