"""Covariance between any two frames of a smoothed track and the relative motion between them (aar_track_smooth_relative).
Needs a real MI355X.

Yardstick: numpy.linalg.inv of the dense H built from the blocks aar_track_smooth_system2 returned at mu = 0 for the same inputs (the practice
of the covariance tests).  Bars:
  cross_cov   largest entry error over the largest entry of the yardstick <= 10 eps kappa_2(H), at every lag (the project's bar for an inverse)
  rel         against the restated between (tests/smooth_restated.py): <= 1e-12, section 25's bar for motions
  rel_cov     against the restated J Sigma J^T on the dense inverse (tests/smooth_relative_restated.py): <= 10 eps kappa_2(H) of the largest
              entry among the four summands -- the sum cancels for strongly correlated frames, so it is not compared to its own size
Measured on the MI355X: DESIGN.md section 35 has the multiples of eps kappa by lag.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_cv_restated as cv
import smooth_fit_cases as fc
import smooth_relative_cases as rc
import smooth_relative_restated as rr
from conftest import PKG, ROOT
from test_gpu_track_smooth import _golden_track, _problem

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SROT, STRANS = rc.SROT, rc.STRANS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _frames(ds, x):
    n0 = sc.ns(ds)
    return np.asarray(x)[n0:n0 + 6 * ds.num_frames].reshape(ds.num_frames, 6)


def _yardstick(p, x0, kw):
    """(Sigma [6F, 6F], kappa_2(H)) from the device's own blocks at mu = 0"""
    gd, go, go2, _, _, cost = p.track_smooth_system2(x0, SROT, STRANS, 0.0, **kw)
    H = cv.dense(gd, go, go2)
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    return np.linalg.inv(H), float(ev[-1] / ev[0]), cost


def _held(tag, ds, x0, pairs, Sigma, kappa, got):
    """items 1, 3 and 4 on one answer; returns the largest errors in units of eps kappa: (cross_cov by lag {lag: e}, rel_cov)"""
    cc, rel, rcv = got
    z = _frames(ds, x0)
    big = float(np.abs(Sigma).max())
    bar = 10 * EPS * kappa
    by_lag, e_rel, e_cov = {}, 0.0, 0.0
    for q, (a, b) in enumerate(np.asarray(pairs)):
        Sab, Saa, Sbb = rr.block(Sigma, a, b), rr.block(Sigma, a, a), rr.block(Sigma, b, b)
        e = float(np.abs(cc[q] - Sab).max() / big)
        by_lag[abs(a - b)] = max(by_lag.get(abs(a - b), 0.0), e)
        if a == b:
            assert not rel[q].any() and not rcv[q].any(), (a, b)
            continue
        e_rel = max(e_rel, float(np.abs(rel[q] - rr.rel(z[a], z[b])).max()))
        terms = rr.summands(z[a], z[b], Saa, Sbb, Sab)
        e_cov = max(e_cov, float(np.abs(rcv[q] - sum(terms)).max() / max(np.abs(t).max() for t in terms)))
    lags = sorted(by_lag)
    print("%s: kappa %.3e, %d pairs; cross_cov in eps kappa by lag: %s; rel %.2e; rel_cov %.4f eps kappa" %
          (tag, kappa, len(pairs), " ".join("%d:%.4f" % (l, by_lag[l] / (EPS * kappa)) for l in lags), e_rel, e_cov / (EPS * kappa)))
    assert max(by_lag.values()) <= bar, (by_lag, bar)
    assert e_rel <= 1e-12, e_rel
    assert e_cov <= bar, (e_cov, bar)
    assert np.array_equal(rcv, np.swapaxes(rcv, 1, 2))
    return by_lag, e_cov


def _check_report(rep, ds, cost, pairs, model, cov_launches):
    F = ds.num_frames
    assert rep["num_residuals"] == 8 * ds.num_obs + 6 * max(F - 1, 0) and rep["num_vars"] == 6 * F
    assert (rep["data_cost"], rep["prior_cost"]) == cost
    dof = rep["num_residuals"] - rep["num_vars"]
    np.testing.assert_allclose(rep["sigma2"], (cost[0] + cost[1]) / dof if dof > 0 else 0.0, rtol=1e-15)
    d, c, m = rr.counts(pairs, model)
    assert (rep["num_pairs"], rep["num_direct"], rep["num_chained"], rep["max_lag"]) == (len(pairs), d, c, m)
    # the covariance call's chain, the lag-three blocks from four frames on, the gains where a chain has an inner node to invert, the queries
    nodes = (F + 1) // 2 if model == "cv" else F
    assert rep["launches"] == cov_launches + (model == "cv" and F >= 4) + (c > 0 and nodes > 2) + 1 and rep["seconds"] > 0


# ---- 1, 3, 4. every pair against the dense inverse ----
@pytest.mark.parametrize("F", rc.SIZES)
@pytest.mark.parametrize("model", ["rw", "cv"])
def test_every_pair_against_the_dense_inverse(model, F):
    ds = rc.dataset(F)
    x0 = sc.track_start(ds)
    kw = dict(frame_time=rc.times(F), **rc.MODELS[model])
    pairs = rc.all_pairs(F)
    with aar.Problem(ds) as p:
        Sigma, kappa, cost = _yardstick(p, x0, kw)
        got = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
        cov = p.track_smooth_covariance2(x0, SROT, STRANS, lag2=model == "cv", **kw)
    assert got[0].shape == (F * F, 6, 6) and got[1].shape == (F * F, 6) and got[2].shape == (F * F, 6, 6)
    _held("%s F %d" % (model, F), ds, x0, pairs, Sigma, kappa, got[:3])
    _check_report(got[3], ds, cost, pairs, model, cov[-1]["launches"])


@pytest.mark.parametrize("model", ["rw", "cv"])
def test_above_the_single_launch_reduction(model):
    F = rc.BIG
    ds = rc.big_dataset()
    x0 = sc.track_start(ds)
    kw = dict(frame_time=rc.times(F), **rc.MODELS[model])
    pairs = rc.big_pairs()
    lag = np.abs(pairs[:, 0] - pairs[:, 1])
    assert [0, F - 1] in pairs.tolist() and [1, F - 1] in pairs.tolist() and 4 in lag and 5 in lag and len(pairs) == 64
    with aar.Problem(ds) as p:
        Sigma, kappa, cost = _yardstick(p, x0, kw)
        got = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
        cov = p.track_smooth_covariance2(x0, SROT, STRANS, lag2=model == "cv", **kw)
    _held("%s F %d" % (model, F), ds, x0, pairs, Sigma, kappa, got[:3])
    _check_report(got[3], ds, cost, pairs, model, cov[-1]["launches"])
    assert cov[-1]["launches"] > (4 if model == "rw" else 5)          # the reduction ran levels in launches of their own


@pytest.mark.parametrize("model", ["rw", "cv"])
def test_huber_problem(model):
    ds, _ = _golden_track("g_track_cfg2_huber")
    x0 = np.array(ds.x_full)
    F = ds.num_frames
    kw = rc.MODELS[model]
    rng = np.random.default_rng(8)
    pairs = np.vstack([rng.integers(0, F, size=(40, 2)), [(0, F - 1), (F - 1, 0), (3, 3)]]).astype(np.int32)
    with _problem(ds, 1.0) as p:
        Sigma, kappa, cost = _yardstick(p, x0, kw)
        got = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
    _held("huber %s F %d" % (model, F), ds, x0, pairs, Sigma, kappa, got[:3])
    with _problem(ds, None) as p:
        plain = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
    assert got[3]["data_cost"] < plain[3]["data_cost"] and not np.array_equal(got[0], plain[0])          # the weights are in H and in the cost
    assert np.array_equal(got[1], plain[1])                                                               # ... and not in the motion


def test_random_walk_with_expected_motions():
    F = 33
    ds = rc.dataset(F)
    x0 = sc.track_start(ds)
    kw = dict(frame_time=rc.times(F), rel_motion=fc.rel_motion(F), model="rw")
    pairs = rc.all_pairs(F)
    with aar.Problem(ds) as p:
        Sigma, kappa, cost = _yardstick(p, x0, kw)
        got = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
        plain = p.track_smooth_relative(x0, SROT, STRANS, pairs, frame_time=rc.times(F), model="rw")
    _held("rw rel_motion F %d" % F, ds, x0, pairs, Sigma, kappa, got[:3])          # (rel is held to the plain between there)
    assert np.array_equal(got[1], plain[1]) and not np.array_equal(got[0], plain[0])          # rel_motion changes H, not rel


# ---- 2. bits ----
@pytest.mark.parametrize("model", ["rw", "cv"])
def test_bits(model):
    F = 33
    ds = rc.dataset(F)
    x0 = sc.track_start(ds)
    keep = np.array(x0)
    kw = dict(frame_time=rc.times(F), **rc.MODELS[model])
    pairs = rc.all_pairs(F)
    a, b = pairs[:, 0], pairs[:, 1]
    with aar.Problem(ds) as p:
        s0 = p.track_smooth(x0, SROT, STRANS, **kw)
        cc, rel, rcv, rep = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
        again = p.track_smooth_relative(x0, SROT, STRANS, pairs, **kw)
        S, R, R2, _ = p.track_smooth_covariance2(x0, SROT, STRANS, lag2=model == "cv", **kw)
        R3 = p.track_smooth_lag3(x0, SROT, STRANS, **kw) if model == "cv" else None
        s1 = p.track_smooth(x0, SROT, STRANS, **kw)
        # the other queries shuffled, duplicated, removed
        rng = np.random.default_rng(2)
        order = rng.permutation(len(pairs))
        shuffled = p.track_smooth_relative(x0, SROT, STRANS, pairs[order], **kw)
        some = np.sort(rng.choice(len(pairs), size=40, replace=False))
        twice = p.track_smooth_relative(x0, SROT, STRANS, np.vstack([pairs[some], pairs[some]]), **kw)
        alone = [p.track_smooth_relative(x0, SROT, STRANS, pairs[q:q + 1], **kw) for q in (F - 1, F * (F - 1), 5 * F + 9)]
        if model == "rw":
            old = p.track_smooth_relative(x0, SROT, STRANS, pairs, frame_time=rc.times(F))          # the struct without the model fields
    assert np.array_equal(x0, keep)
    for u, v in zip(s0, s1):                                          # aar_track_smooth before and after: no LM state is left behind
        if isinstance(u, dict):
            assert all(k == "seconds" or u[k] == v[k] for k in u)
        else:
            assert np.array_equal(u, v)
    for u, v in zip((cc, rel, rcv), again[:3]):
        assert np.array_equal(u, v)
    assert all(rep[k] == again[3][k] for k in rep if k != "seconds")
    sq = lambda m: m.reshape(F, F, *m.shape[1:])
    CC, REL, RCV = sq(cc), sq(rel), sq(rcv)
    idx = np.arange(F)
    assert np.array_equal(CC[idx, idx], S)                            # lag 0 is frame_cov
    assert np.array_equal(CC[idx[:-1], idx[1:]], R)                   # lag 1 is lag_cov
    if model == "cv":
        assert np.array_equal(CC[idx[:-2], idx[2:]], R2)              # lag 2 is lag2_cov
        assert np.array_equal(CC[idx[:-3], idx[3:]], R3)              # lag 3 is aar_track_smooth_lag3
    assert np.array_equal(CC, CC.transpose(1, 0, 3, 2))               # (b, a) is the transpose of (a, b)  [the diagonal blocks are symmetric]
    assert np.array_equal(RCV, RCV.transpose(0, 1, 3, 2))             # rel_cov is symmetric
    assert not REL[idx, idx].any() and not RCV[idx, idx].any()        # a = b: zeros
    assert np.all(np.isfinite(cc)) and np.all(np.isfinite(rel)) and np.all(np.isfinite(rcv))
    for u, v in zip((cc, rel, rcv), shuffled[:3]):
        assert np.array_equal(u[order], v)
    for u, v in zip((cc, rel, rcv), twice[:3]):
        assert np.array_equal(u[some], v[:40]) and np.array_equal(u[some], v[40:])
    for q, one in zip((F - 1, F * (F - 1), 5 * F + 9), alone):
        assert all(np.array_equal(u[q], v[0]) for u, v in zip((cc, rel, rcv), one[:3])), q
    if model == "rw":
        assert all(np.array_equal(u, v) for u, v in zip((cc, rel, rcv), old[:3]))


# ---- 5. the reason for the feature ----
@pytest.mark.parametrize("model", ["rw", "cv"])
def test_static_object_most_distant_pair(model):
    """Measured on the MI355X: see DESIGN.md section 35 for the recorded ratios."""
    ds, x0, zt = sc.static_object(64)
    F = ds.num_frames
    kw = rc.MODELS[model]
    pairs = np.array([(0, F - 1)], dtype=np.int32)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs = p.track_smooth(xt, SROT, STRANS, **kw)[0]
        Sigma, kappa, cost = _yardstick(p, xs, kw)
        got = p.track_smooth_relative(xs, SROT, STRANS, pairs, **kw)
        S = p.track_smooth_covariance2(xs, SROT, STRANS, lag2=model == "cv", **kw)[0]
    _held("static object %s" % model, ds, xs, pairs, Sigma, kappa, got[:3])
    z = _frames(ds, xs)
    Saa, Sbb, Sab = rr.block(Sigma, 0, 0), rr.block(Sigma, F - 1, F - 1), rr.block(Sigma, 0, F - 1)
    dense = np.trace(rr.rel_cov(z[0], z[F - 1], Saa, Sbb, Sab)) / np.trace(Saa + Sbb)
    dev = np.trace(got[2][0]) / np.trace(S[0] + S[F - 1])
    print("static object %s, frames 0 and %d: tr(rel_cov) / tr(Sigma_aa + Sigma_bb) = %.6f from the dense inverse, %.6f from the device" %
          (model, F - 1, dense, dev))


# ---- 6. errors and edges ----
def _raw(p, x0, pairs, kw, cross=True, rel=True, rcov=True, report=True, struct_size=None, fill=7.0):
    """the C call with sentinel-filled outputs: (code, cross_cov, rel, rel_cov, report struct)"""
    x = np.array(p._x(x0), dtype=np.float64)
    keep = x.copy()
    spar = aar.SmoothParams(SROT, STRANS, None, None, None, **kw)
    fa, fb = aar._pairs(pairs)
    Q = len(fa)
    cc, rl, rc_ = np.full((max(Q, 1), 6, 6), fill), np.full((max(Q, 1), 6), fill), np.full((max(Q, 1), 6, 6), fill)
    rep = aar.CSmoothRelativeReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep) if struct_size is None else struct_size
    ip = C.POINTER(C.c_int32)
    code = aar.lib().aar_track_smooth_relative(p.handle, aar._dptr(x), C.byref(spar.c), Q, fa.ctypes.data_as(ip) if Q else None,
                                               fb.ctypes.data_as(ip) if Q else None, aar._dptr(cc) if cross else None, aar._dptr(rl) if rel else None,
                                               aar._dptr(rc_) if rcov else None, C.byref(rep) if report else None)
    assert np.array_equal(x, keep)
    return code, cc, rl, rc_, rep


@pytest.mark.parametrize("model", ["rw", "cv"])
def test_errors_and_edges(model):
    kw = rc.MODELS[model]
    F = 9
    ds = rc.dataset(F)
    x0 = sc.track_start(ds)
    pairs = [(0, 8), (8, 0), (2, 2), (1, 2), (3, 8)]
    with aar.Problem(ds) as p:
        code, cc, rl, rcv, rep = _raw(p, x0, pairs, kw)
        assert code == 0 and not np.any(cc == 7.0) and not np.any(rl[[0, 1, 3, 4]] == 7.0) and not np.any(rcv == 7.0)
        # NULL outputs one at a time, and all at once
        for off in (dict(cross=False), dict(rel=False), dict(rcov=False), dict(report=False), dict(cross=False, rel=False, rcov=False, report=False)):
            code, cc2, rl2, rcv2, rep2 = _raw(p, x0, pairs, kw, **off)
            assert code == 0, off
            assert np.array_equal(cc2, cc) if off.get("cross", True) else np.all(cc2 == 7.0)
            assert np.array_equal(rl2, rl) if off.get("rel", True) else np.all(rl2 == 7.0)
            assert np.array_equal(rcv2, rcv) if off.get("rcov", True) else np.all(rcv2 == 7.0)
            if off.get("report", True):
                assert rep2.sigma2 == rep.sigma2 and rep2.num_pairs == 5 and rep2.max_lag == 8
        # a caller compiled against a shorter report
        cut = aar.CSmoothRelativeReport.num_pairs.offset
        code, _, _, _, rep3 = _raw(p, x0, pairs, kw, struct_size=cut)
        assert code == 0 and rep3.struct_size == cut and rep3.sigma2 == rep.sigma2
        assert bytes(bytearray(rep3)[cut:]) == b"\x55" * (C.sizeof(rep3) - cut)
        # n_pairs = 0: no output written
        code, cc0, rl0, rcv0, rep0 = _raw(p, x0, np.zeros((0, 2)), kw)
        assert code == 0 and np.all(cc0 == 7.0) and np.all(rl0 == 7.0) and np.all(rcv0 == 7.0) and rep0.num_pairs == 0 and rep0.launches == 0
        e0 = p.track_smooth_relative(x0, SROT, STRANS, np.zeros((0, 2)), **kw)
        assert e0[0].shape == (0, 6, 6) and e0[1].shape == (0, 6) and e0[2].shape == (0, 6, 6)
        # indices out of range, on both sides, named
        for bad, what in (([(0, 8), (9, 0)], "frame_a[1] = 9"), ([(-1, 0)], "frame_a[0] = -1"), ([(0, 9)], "frame_b[0] = 9"), ([(0, 1), (1, -2)], "frame_b[1] = -2")):
            code, cc2, rl2, rcv2, _ = _raw(p, x0, bad, kw)
            assert code == aar.AAR_ERR_INVALID and what in aar.lib().aar_last_error().decode(), what
            assert np.all(cc2 == 7.0) and np.all(rl2 == 7.0) and np.all(rcv2 == 7.0)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_relative(x0, -1.0, STRANS, pairs, **kw)
        assert e.value.code == aar.AAR_ERR_INVALID
    # nothing seen anywhere: a numeric error, the outputs untouched
    none = sc.without_frames(aar.synth(2, num_frames=6), range(6))
    assert none.num_obs == 0
    with aar.Problem(none) as p:
        code, cc, rl, rcv, _ = _raw(p, sc.track_start(none), [(0, 5), (1, 1)], kw)
        assert code == aar.AAR_ERR_NUMERIC and np.all(cc == 7.0) and np.all(rl == 7.0) and np.all(rcv == 7.0)
    # one frame
    one = aar.synth(2, num_frames=1)
    with aar.Problem(one) as p:
        S = p.track_smooth_covariance2(sc.track_start(one), SROT, STRANS, lag2=model == "cv", **kw)[0]
        cc, rl, rcv, rep = p.track_smooth_relative(sc.track_start(one), SROT, STRANS, [(0, 0), (0, 0)], **kw)
        assert np.array_equal(cc[0], S[0]) and np.array_equal(cc[1], S[0]) and not rl.any() and not rcv.any()
        assert (rep["num_direct"], rep["num_chained"], rep["max_lag"]) == (2, 0, 0)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_relative(sc.track_start(one), SROT, STRANS, [(0, 1)], **kw)
        assert e.value.code == aar.AAR_ERR_INVALID and "frame_b[0] = 1" in str(e.value)


def test_unsupported_behind_a_communicator():
    ds, _ = _golden_track("g_track_cfg2")
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            for kw in rc.MODELS.values():
                with pytest.raises(aar.AarError) as e:
                    p.track_smooth_relative(ds.x_full, SROT, STRANS, [(0, 1)], **kw)
                assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    finally:
        comm.close()
        group.close()


# ---- 7. the upper layers ----
def _kv(stdout):
    return dict(l.split(" = ") for l in stdout.splitlines() if " = " in l)


def parse_relative_yaml(path):
    """(sigma2, relative_to, frame ids [n], baselines [n], rel [n, 6], covariance [n, 6, 6]) of final.smooth_relative.yaml"""
    text = open(path).read()
    head, body = text.split("relative_motions:\n")
    sigma2 = float(head.split("sigma2: ")[1].split("\n")[0])
    base = int(head.split("relative_to: ")[1].split("\n")[0])
    ids, dt, rel, cov = [], [], [], []
    for item in body.split("   - { frame: ")[1:]:
        ids.append(int(item.split(",")[0]))
        dt.append(float(item.split("baseline: ")[1].split(",")[0]))
        rel.append([float(v) for v in item.split("rel: [")[1].split("]")[0].split(",")])
        cov.append([float(v) for v in item.split("data:[")[1].split("]")[0].split(",")])
    return sigma2, base, np.array(ids), np.array(dt), np.array(rel), np.array(cov).reshape(-1, 6, 6)


@pytest.mark.parametrize("model", ["rw", "cv"])
def test_mapper_track_smooth_relative(tmp_path, model):
    exe = str(tmp_path / "smooth_relative_mapper_main")
    cc_ = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_relative_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                          "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr
    ds = aar.synth(2)
    F = ds.num_frames
    pairs = [(0, F - 1), (F - 1, 0), (7, 7), (7, 8), (9, 7), (7, 10), (8, 12), (40, 13)]
    kw = rc.MODELS[model]
    run = subprocess.run([exe, "2", model, repr(SROT), repr(STRANS), repr(kw.get("sigma_rot0", 0.0)), repr(kw.get("sigma_trans0", 0.0))] +
                         [str(v) for ab in pairs for v in ab], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = _kv(run.stdout)
    x = np.array([float(v) for v in kv["x"].split()])          # the pose vector the driver's call ran at, exactly
    assert x.shape == np.asarray(ds.x_full).shape
    ft = np.asarray(ds.frame_ids, dtype=np.float64)
    with aar.Problem(ds) as p:
        cc, rel, rcv, rep = p.track_smooth_relative(x, SROT, STRANS, pairs, frame_time=ft, **kw)
    assert [int(kv[k]) for k in ("pairs", "direct", "chained", "max_lag", "launches")] == \
        [rep[k] for k in ("num_pairs", "num_direct", "num_chained", "max_lag", "launches")]
    assert float(kv["sigma2"]) == rep["sigma2"]
    for k in range(len(pairs)):
        got = [np.array([float(v) for v in kv["%s%d" % (name, k)].split()]) for name in ("cross", "rel", "relcov")]
        assert np.array_equal(got[0].reshape(6, 6), cc[k]) and np.array_equal(got[1], rel[k]) and np.array_equal(got[2].reshape(6, 6), rcv[k]), k


@pytest.mark.parametrize("model", ["rw", "cv"])
def test_find_solution_relative_to_switch(tmp_path, model):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # as tests/test_gpu_track_smooth_query.py: the recording is cut before config 2's frames that turn through pi
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    kw = rc.MODELS[model]
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    smooth = ["-smooth", repr(SROT), repr(STRANS)] + (["-cv", repr(kw["sigma_rot0"]), repr(kw["sigma_trans0"])] if model == "cv" else [])
    ref_id = int(cut.frame_ids[5])
    run = subprocess.run(base + smooth + ["-relative-to", str(ref_id)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, AAR_DETERMINISTIC="1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert len([l for l in run.stdout.splitlines() if l.startswith("smooth-relative: ")]) == 1, run.stdout
    path = os.path.join(folder, "final.smooth_relative.yaml")
    sigma2, rid, ids, dt, rel, blk = parse_relative_yaml(path)
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    F = got.num_frames
    ft = np.asarray(got.frame_ids, dtype=np.float64)
    assert F == FK and rid == ref_id and np.array_equal(ids, got.frame_ids) and np.array_equal(dt, ft - ft[5])
    with aar.Problem(got) as p:
        _, rel_p, rcv_p, rep = p.track_smooth_relative(got.x_full, SROT, STRANS, [(5, f) for f in range(F)], frame_time=ft, **kw)
    want = rep["sigma2"] * rcv_p
    print("%s: sigma2 %.17g against %.17g; rel differs by %.3e, covariance by %.3e of %.3e" %
          (model, sigma2, rep["sigma2"], np.abs(rel - rel_p).max(), np.abs(blk - want).max(), np.abs(want).max()))
    assert sigma2 == rep["sigma2"] and np.array_equal(rel, rel_p) and np.array_equal(blk, want)
    assert not rel[5].any() and not blk[5].any()
    # refused with the usage message: without -smooth, together with -live, without its value, a frame the recording does not have
    os.remove(path)
    for bad in (base + ["-relative-to", str(ref_id)], base + ["-live", "0", "-relative-to", str(ref_id)], base + smooth + ["-relative-to"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-relative-to" in run.stdout and "smooth-relative: " not in run.stdout, run.stdout
        assert not os.path.exists(path)
    run = subprocess.run(base + smooth + ["-relative-to", "100000"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 6 and "no frame with id 100000" in run.stderr and not os.path.exists(path)
