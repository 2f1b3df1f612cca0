"""Certificates of aar_problem_covariance -- S^-1 and the frame blocks -- in every launch shape of the chain it reuses, against the float64
restatement of tests/covariance_certificate.py built from the DEVICE'S OWN dense normal equations (the observation passes are out of the
comparison; what is left is frame inverse + Schur complement + k_cov_stage + LDL^T + k_cov_gather + X = L^-1 + X^T D^-1 X + k_cov_frames).
Needs a real MI355X.

Every problem is created with solver="direct" unless stated and runs at ds.x_full.  Every test asserts its premise first: from the data set, from
solver_stats(), or from the launch counts of the covariance call itself (aar_get_kernel_times): the staged system has one tile more than the
LM path's, so the counts are _ldl_expected(nT + 1, ...).  A data set's float64 system is built once, from the first problem that asks for it:
problems of other launch shapes on the same set are certified against that H -- theirs differs in summation order only, which is inside M.

Which branch of k_cov_gather a block column of L comes from: Lp where nT + 1 - tj - 1 <= AAR_FUSED_PANEL (k_ldl_panel launched for it), the
staged system in place otherwise (k_ldl_trsm launched for it).  The in-place branch, the look-ahead path (k_ldl_trsm launches without a
k_ldl_update of their own) and k_schur_mfma at mu = 0 are each asserted by a premise of test_gather_branches / test_tile_sweep.

Ratios: every certified call's worst entity-block ratio and worst frame ratio are collected per family and printed when the module finishes
(run with -s).  The float64 routes' ratios on the same sets are in tests/test_covariance_certificate_host.py (entity part below 2.3e-5 of the
bar, frame part below 3.6e-2); NO DEVICE RATIO IS RECORDED YET.
"""
import numpy as np
import pytest

import aar
import covariance_certificate as cc
import direct_cases as dc
from covariance_cases import CASES, case_keywords
from direct_cases import ldl_env as _ldl_env, ldl_expected as _ldl_expected, run_ranks as _run_ranks

pytestmark = pytest.mark.gpu

RATIOS = {}                # family -> [(entity ratio, frame ratio)]
_SYS = {}                  # the current data-set key -> (CovSystem, the device's sum of squares): one system at a time


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_report():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")
    yield
    print("\ncovariance certificate ratios (family: calls, worst, median entity ratio; worst, median frame ratio)")
    for fam, v in sorted(RATIOS.items()):
        a = np.array(v)
        print("  %-18s %4d  %.3e  %.3e   %.3e  %.3e" % (fam, len(a), a[:, 0].max(), np.median(a[:, 0]), a[:, 1].max(), np.median(a[:, 1])))


def _x0(p, ds, intr):
    return p.x_with_intrinsics(ds.x_full) if intr else np.asarray(ds.x_full, dtype=np.float64)


def _system(key, p, ds, opt=(True, True, True), intr=False, fixed=None):
    if key not in _SYS:
        _SYS.clear()
        H, _, ss = p.eval_normal_equations(_x0(p, ds, intr))      # (the device's H carries the Huber weights and the priors' blocks)
        _SYS[key] = (cc.CovSystem(ds, H, opt, intr, **(fixed or {})), ss)
    return _SYS[key]


def _check(family, cs, ss, cv, p, ds, what, partial=False):
    a = cc.certify_entity(cs, cv.entity_cov, what)
    b = cc.certify_frames(cs, cv.entity_cov, cv.frames, what, partial=partial)
    cc.certify_report(cs, cv, ss, p.num_vars, 8 * ds.num_obs, what)
    for k, (kind, idx, off, sz) in enumerate(cs.blocks):      # the diagonal blocks are the dense output's
        assert np.array_equal(cv.entity_diag[k], cv.entity_cov[off:off + sz, off:off + sz], equal_nan=True), (what, kind, idx)
    RATIOS.setdefault(family, []).append((a["ratio"], b["ratio"]))
    return a, b


def _certify(family, key, p, ds, opt=(True, True, True), intr=False, fixed=None, what=""):
    """certify one covariance call of problem p at its start point; returns the Covariance"""
    cs, ss = _system(key, p, ds, opt, intr, fixed)
    cv = p.covariance(_x0(p, ds, intr), dense=True)
    _, b = _check(family, cs, ss, cv, p, ds, "%s %s %s" % (family, key, what))
    assert cv.frames_written == ds.num_frames and len(b["certified"]) == len(cs.frames_live)
    return cv


def _problem(ds, **kw):
    kw.setdefault("solver", "direct")
    return aar.Problem(ds, **kw)


def _case(name, **over):
    """(ds, Problem keywords, certificate keywords) of a case of the host module"""
    make, kw = CASES[name]
    ds = make()
    opt, intr, hub, fixed, pri = case_keywords(ds, kw, np.asarray(ds.x_full, dtype=np.float64))
    pk = dict(optimize=opt, intrinsics=intr, with_huber=hub, **fixed)
    if pri:
        pk["priors"] = pri
    pk.update(over)
    return ds, pk, dict(opt=opt, intr=intr, fixed=fixed)


def _launch_counts(p, x):
    """launches of one covariance call"""
    p.set_kernel_profiling(True)
    before = {k: v[1] for k, v in p.kernel_times().items()}
    p.covariance(x)
    cnt = {k: v[1] - before[k] for k, v in p.kernel_times().items()}
    p.set_kernel_profiling(False)
    return cnt


# ---------------------------------------------------------------------------------------------------------------------------------------------
# tile sweep: nT = 1 .. 14, both Schur kernels
@pytest.mark.parametrize("nT", list(range(1, 15)))
@pytest.mark.parametrize("mfma", ["0", "1"])
def test_tile_sweep(nT, mfma, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", mfma)
    ds = dc.sweep_ds(nT)
    assert dc.tiles_of(ds) == nT and 6 * (ds.num_cams + ds.num_markers) == 96 * nT - 18
    with _problem(ds) as p:
        # premise (mfma = 1), as far as it can be observed: the problem is neither deterministic nor PCG, has frames, and the dense panels of the
        # MFMA kernel (2 F pad32(A + 1) 288 bytes) are far below any memory budget -- the conditions under which ba_capi.hip (schur_mfma) builds
        # the MFMA work list when the switch says so.  WHICH Schur kernel then ran is known from reading launch_schur only: aar_get_kernel_times
        # bills both kernels as k_schur.  The covariance call runs the problem's Schur kernel at mu = 0.
        st = p.solver_stats()
        assert not st["deterministic"] and st["solver"] == "direct" and ds.num_frames > 0
        assert 2 * ds.num_frames * (-(-(ds.num_cams + ds.num_markers + 1) // 32) * 32) * 288 < 64 << 20
        _certify("sweep mfma=" + mfma, "sweep%d" % nT, p, ds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# k_cov_gather: block columns of L from Lp, from the staged system in place, and both; look-ahead on and off
@pytest.mark.parametrize("nT", [1, 2, 4, 5, 8, 14])
@pytest.mark.parametrize("fused", [0, 2, 3, 5])
@pytest.mark.parametrize("lookahead", [0, 1])
def test_gather_branches(nT, fused, lookahead, monkeypatch):
    _ldl_env(monkeypatch, fused, lookahead)
    ds = dc.sweep_ds(nT)
    with _problem(ds) as p:
        cnt = _launch_counts(p, np.asarray(ds.x_full, dtype=np.float64))
        want = _ldl_expected(nT + 1, fused, lookahead, 1)
        assert cnt["k_ldl_diag"] == nT + 1 and all(cnt[n] == want[n] for n in ("k_ldl_panel", "k_ldl_trsm", "k_ldl_update")), (cnt, want)
        inplace = nT + 1 - 1 > fused                     # block column 0 has nT tiles below the diagonal
        assert (cnt["k_ldl_trsm"] > 0) == inplace and (cnt["k_ldl_panel"] > 0) == (fused > 0)
        if lookahead and nT + 1 - 1 > max(fused, 1):
            assert cnt["k_ldl_update"] < cnt["k_ldl_trsm"]          # the look-ahead path ran
        _certify("gather branches", "sweep%d" % nT, p, ds, what="fused %d lookahead %d" % (fused, lookahead))


@pytest.mark.parametrize("nT", [1, 2])
def test_back_substitution_as_its_own_launch(nT, monkeypatch):
    _ldl_env(monkeypatch, bs_rides=0)
    ds = dc.sweep_ds(nT)
    with _problem(ds) as p:
        cnt = _launch_counts(p, np.asarray(ds.x_full, dtype=np.float64))
        assert cnt["k_ldl_backsolve"] == 1 and cnt["k_ldl_diag"] == nT + 1, cnt
        _certify("gather branches", "sweep%d" % nT, p, ds, what="AAR_BS_RIDES=0")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# masks
@pytest.mark.parametrize("cams,row", [(16, 96), (15, 90), (34, 204)])
def test_root_marker_rows_at_tile_boundaries(cams, row):
    ds, pk, ck = _case("gauge_c%d" % cams)
    assert dc.tiles_of(ds) == 3 and 6 * (ds.num_cams + ds.root_marker) == row      # first rows of tile 1 / last rows of tile 0 (and of a 32-row block) / inside tile 2
    with _problem(ds, **pk) as p:
        _certify("masks", "gauge_c%d" % cams, p, ds, **ck)


@pytest.mark.parametrize("which", ["cams_off", "markers_off", "fixed"])
@pytest.mark.parametrize("tiles", [3, 5])
def test_groups_off_and_caller_fixed_entities(tiles, which):
    ds, pk, ck = _case("%s_%d" % (which, tiles))
    assert dc.tiles_of(ds) == tiles and ds.num_cams == 16
    with _problem(ds, **pk) as p:
        cv = _certify("masks", "%s_%d" % (which, tiles), p, ds, **ck)
        cs = _SYS["%s_%d" % (which, tiles)][0]
        unseen = sum(1 for m, k in enumerate(dc.frames_per_marker(ds)) if k == 0 and m != ds.root_marker) if ck["opt"][1] else 0
        dead = 6 * unseen + (18 if which == "fixed" else 0)      # (the five-tile set has a marker no frame sees)
        assert (~cs.live).sum() == dead and np.isnan(cv.entity_cov).any() == (dead > 0)


def test_a_marker_seen_nowhere_and_one_seen_once():
    ds, pk, ck = _case("worklist_unseen")
    fpm = dc.frames_per_marker(ds)
    assert fpm[7] == 0 and fpm[11] == 1
    with _problem(ds, **pk) as p:
        cv = _certify("masks", "worklist_unseen", p, ds, **ck)
        k = ds.num_cams - 1 + 7 - (7 > ds.root_marker)
        assert np.isnan(cv.entity_diag[k]).all() and sum(np.isnan(b).all() for b in cv.entity_diag) == 1


def test_a_frame_without_observations():
    ds, pk, ck = _case("empty_frame")
    assert dc.frame_entity_counts(ds)[5] == 0 and min(k for f, k in enumerate(dc.frame_entity_counts(ds)) if f != 5) > 0
    with _problem(ds, **pk) as p:
        cv = _certify("masks", "empty_frame", p, ds, **ck)
        assert np.isnan(cv.frames[5]).all() and np.isfinite(np.delete(cv.frames, 5, axis=0)).all()


def test_a_frame_that_sees_only_the_roots():
    ds, f = dc.roots_only_frame(dc.worklist_ds(60))
    _, pk, ck = _case("roots_only_frame")
    assert dc.frame_entity_counts(ds)[f] == 2
    with _problem(ds, **pk) as p:
        cv = _certify("masks", "roots_only_frame", p, ds, **ck)
        cs = _SYS["roots_only_frame"][0]
        k = list(cs.frames_live).index(f)
        assert not cs.rs.W64[:, k, :].any()                        # premise: every W row of the frame is a gauge row, so Sigma_ff = V_f^-1
        np.testing.assert_allclose(cv.frames[f], cs.rs.Vinv[k], rtol=0, atol=cc.frame_gamma(2) * cs.rs.frame_conds()[k] * np.linalg.norm(cs.rs.Vinv[k]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# k_cov_frames: slot pairs on both sides of one round of 64 lanes, frames of more than 64 slots, slots with idle rows
@pytest.mark.parametrize("name", ["small_frames", "small_frames_intr", "small_frames_intr_fixture", "wide_84", "wide_92"])
def test_frame_kernel_slot_counts(name, monkeypatch):
    ds, pk, ck = _case(name)
    kf = dc.frame_entity_counts(ds, intrinsics=ck["intr"])
    if name == "small_frames":
        assert kf[:5] == dc.SMALL_TARGETS
    elif name == "small_frames_intr":
        assert set(dc.SMALL_TARGETS_INTRINSICS) <= set(kf)
    elif name == "small_frames_intr_fixture":
        assert set(dc.SMALL_TARGETS_INTRINSICS[:3]) <= set(kf) and {12, 13} <= set(kf)      # (cut to 3, 6, 10; its own frames have 12 and 13: no frame can be cut to 11)
    else:
        assert max(kf) > 64 and min(kf) < 30 and any(30 < k < 60 for k in kf) and any(60 < k <= 64 for k in kf), kf
    pairs = [k * (k + 1) // 2 for k in kf]
    if name.startswith("small_frames"):
        assert any(q < 64 for q in pairs) and any(64 < q < 128 for q in pairs), pairs
    with _problem(ds, **pk) as p:
        _certify("frame kernel", name, p, ds, **ck)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# solvers: the call takes the direct chain whatever the solver; the fp32 W blocks of a PCG problem must not leak into the frame blocks
@pytest.mark.parametrize("solver", ["pcg", "spcg", "auto"])
def test_solvers(solver, monkeypatch):
    monkeypatch.delenv("AAR_SCHUR_MFMA", raising=False)
    ds = dc.sweep_ds(7)
    with _problem(ds, solver=solver) as p:
        # premise: the solver is the one asked for (AUTO: resolved to one of the three).  A PCG problem builds no MFMA work list (ba_capi.hip,
        # "if (schur_mfma && !P.use_pcg)"), so its covariance call forms S with the output-stationary kernel, k_schur<0>, although the set has
        # more than 96 entities; its solve reads the fp32 Wf blocks, which are allocated for PCG problems only, and the covariance call must not:
        # it asks eval_blocks for the fp64 W (want_w64).  A leak shows in (b): a frame's W rounded to fp32 fails the bar by 1e4 on the host.
        got = p.solver_stats()["solver"]
        assert (got == solver if solver != "auto" else got in ("direct", "spcg", "pcg")) and dc.tiles_of(ds) == 7 and ds.num_cams + ds.num_markers >= 96
        _certify("solvers", "sweep7", p, ds, what=solver)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# variants
@pytest.mark.parametrize("nT", [1, 3, 7])
def test_deterministic_equal_bits_twice_and_across_solvers(nT):
    ds = dc.sweep_ds(nT)
    got = []
    for solver in ("direct", "direct", "spcg", "pcg", "auto"):
        with _problem(ds, solver=solver, deterministic=True) as p:
            assert p.solver_stats()["deterministic"]
            got.append(_certify("deterministic", "sweep%d" % nT, p, ds, what=solver))
    for cv in got[1:]:
        assert np.array_equal(cv.entity_cov, got[0].entity_cov, equal_nan=True) and np.array_equal(cv.frames, got[0].frames)
        assert (cv.sigma2, cv.min_pivot, cv.max_pivot) == (got[0].sigma2, got[0].min_pivot, got[0].max_pivot)


@pytest.mark.parametrize("name", ["huber", "intrinsics", "priors_fixed"])
def test_variants(name):
    ds, pk, ck = _case(name)
    with _problem(ds, **pk) as p:
        cv = _certify("variants", name, p, ds, **ck)
        if name == "intrinsics":
            for blk in cv.entity_diag[-ds.num_cams:]:
                assert blk.shape == (9, 9) and np.isnan(blk[4:, :]).all() and np.isnan(blk[:, 4:]).all() and np.isfinite(blk[:4, :4]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ranks: every rank's entity part is certified, every frame by exactly one rank
@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("world,nT,frames", [(2, 2, None), (3, 5, None), (3, 2, 2)])
def test_ranks(world, nT, frames, pack, monkeypatch):
    monkeypatch.setenv("AAR_PACK_SYSTEM", pack)
    ds, key = (dc.mfma_frames_ds(frames), "mfma_F%d" % frames) if frames else (dc.sweep_ds(nT), "sweep%d" % nT)      # (two frames for three ranks: one has none)
    assert dc.tiles_of(ds) == nT and (ds.num_frames < world) == bool(frames)
    x = np.asarray(ds.x_full, dtype=np.float64)
    with _problem(ds) as p:      # the ONE-rank device H of the same problem: the ranks' sum differs from it in summation order only
        cs, ss = _system(key, p, ds)
        nv = p.num_vars

    def run(comm, rank):
        with aar.Problem(ds, comm=comm, solver="direct") as q:
            return q.covariance(x, dense=True), q.local_obs
    res = _run_ranks(world, run)
    assert (min(r[1] for r in res) == 0) == bool(frames), [r[1] for r in res]
    seen = np.zeros(ds.num_frames, int)
    for r, (cv, _) in enumerate(res):
        class _P:
            num_vars = nv
        _, b = _check("ranks", cs, ss, cv, _P, ds, "world %d rank %d nT %d AAR_PACK_SYSTEM=%s" % (world, r, nT, pack), partial=True)
        assert len(b["certified"]) == cv.frames_written
        seen[b["certified"]] += 1
        assert np.array_equal(cv.entity_cov, res[0][0].entity_cov, equal_nan=True)        # identical bits on every rank
    assert np.all(seen[cs.frames_live] == 1), seen


# ---------------------------------------------------------------------------------------------------------------------------------------------
# state: the call leaves the LM path as it found it
def test_covariance_then_solve_then_covariance():
    ds = dc.sweep_ds(3)
    x = np.asarray(ds.x_full, dtype=np.float64)
    prm = aar.lm_default_params(max_iters=3)
    with _problem(ds, deterministic=True) as p:
        x_fresh, rep_fresh = p.lm_solve(x, params=prm)
    with _problem(ds, deterministic=True) as p:
        c1 = _certify("state", "sweep3", p, ds, what="first call")
        x1, rep1 = p.lm_solve(x, params=prm)
        c2 = _certify("state", "sweep3", p, ds, what="after lm_solve")
    assert rep1["iterations"] == rep_fresh["iterations"] > 0
    assert np.array_equal(x1, x_fresh)                                  # lm_solve after a covariance call: the bits of a fresh problem
    assert np.array_equal(c1.entity_cov, c2.entity_cov, equal_nan=True) and np.array_equal(c1.frames, c2.frames)
    assert (c1.sigma2, c1.min_pivot, c1.max_pivot) == (c2.sigma2, c2.min_pivot, c2.max_pivot)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# g2_small (the set the flat 1e-7 bar sat 10 % above), config 3 whole, config 5 as a slice of its shape
def _bar_terms(cs, i, j):
    """the bar of block (i, j) split by term of M, relative to |Sigma*_ij|: (formation with kappa_f = 1, what kappa_f adds, |L| |D| |L^T|)"""
    e = cs.entity()
    lv = cs.live
    sa = np.abs(np.asarray(e["sigma"], dtype=np.float64))
    rs = cs.rs
    n = len(rs.ent)
    Wa = np.abs(rs.W64)
    T1 = np.einsum("efi,fij->efj", Wa, np.abs(rs.Vinv))
    plain = np.abs(rs.U) + T1.reshape(n, -1) @ Wa.reshape(n, -1).T
    EA = rs.abs_sums()[0]
    out = []
    for M in (plain, EA - plain, cs.M - EA):
        out.append(cs.gamma() * cs.block_norms(sa @ M[np.ix_(lv, lv)] @ sa)[i, j] / e["norms"][i, j])
    return out


@pytest.mark.parametrize("name", ["g2_small", "cfg3", "cfg5_shaped"])
def test_g2_small_config3_and_a_config5_slice(name):
    ds, pk, ck = _case(name)
    with _problem(ds, **pk) as p:
        cv = _certify("full size", name, p, ds, **ck)
        if name == "g2_small":
            # which term of the bar accounts for the 9e-8 of the flat comparison (tests/test_gpu_covariance.py).  That comparison measures against
            # np.linalg.inv of H in float64 and relative to (|Sigma_aa| |Sigma_bb|)^1/2; here the same metric is taken against the refined
            # Sigma*, for the device AND for np.linalg.inv of the device's own H, beside the three terms of the worst block's bar.
            cs = _SYS[name][0]
            e = cs.entity()
            lv = cs.live
            dn = np.sqrt(np.diag(e["norms"]))
            sc = np.where(np.outer(dn, dn) > 0, np.outer(dn, dn), np.inf)

            def flat(sg):
                return cs.block_norms(np.asarray(sg[np.ix_(lv, lv)].astype(np.longdouble) - e["sigma"], dtype=np.float64)) / sc
            dev, ref64 = flat(cv.entity_cov), flat(cc.dense_inverse_route(cs)[0])
            i, j = np.unravel_index(int(np.argmax(dev)), dev.shape)
            t = np.array(_bar_terms(cs, i, j)) * e["norms"][i, j] / sc[i, j]           # the three terms in the flat metric
            covered = ["formation at kappa_f = 1", "kappa_f's share", "|L||D||L^T|"][int(np.argmax(np.cumsum(t) >= dev[i, j]))]
            print("g2_small, flat metric against Sigma*: device worst %.3e in (%s %d, %s %d), np.linalg.inv of H worst %.3e; that block's bar: formation at "
                  "kappa_f = 1 %.3e, kappa_f's share %.3e, |L||D||L^T| %.3e -> covered by: %s; kappa_f max %.3e, cond_2(S) %.3e"
                  % (dev[i, j], *cs.blocks[i][:2], *cs.blocks[j][:2], ref64.max(), t[0], t[1], t[2], covered, cs.rs.frame_conds().max(), e["cond"]))
            # judged: the three terms together cover the device's worst block (the same statement as ratio <= 1, in the flat metric); the flat
            # comparison's figure is then the sum of two float64 errors of this size -- the device's and np.linalg.inv's -- and no fault of the chain
            assert np.cumsum(t)[-1] >= dev[i, j], (dev[i, j], t)
