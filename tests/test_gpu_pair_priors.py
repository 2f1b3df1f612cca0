"""Relative pose priors between two cameras / two markers on the device.  Every reference is independent of the kernel:
the normal equations of a TWIN problem without pair priors (aar_eval_normal_equations at mu = 0) plus the float64 numpy restatement of the
pair terms (tests/pair_priors_restated.py)."""
import threading

import numpy as np
import pytest

import aar
from aar import Problem
from conftest import load_golden
from pair_priors_restated import pair_e, pair_residuals, pair_terms, pose_of
from reduced_system import prior_terms, rodrigues, slot_col, so3_log

pytestmark = pytest.mark.gpu

# Largest relative block error of H_c - H_twin and B_c - B_twin against the restatement over all cases of
# test_normal_equation_blocks_match_the_restatement, measured on the MI355X: 1.68e-13 (the root_end case).  The bar is ten times that.
BLOCK_BAR = 1.7e-12
assert BLOCK_BAR <= 1e-10


def free_entities(ds):
    return [c for c in range(ds.num_cams) if c != ds.root_cam], [m for m in range(ds.num_markers) if m != ds.root_marker]


def random_spd(rng, scale=1.0):
    A = rng.standard_normal((6, 6))
    return scale * (A @ A.T + 6 * np.eye(6))


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def make_pair(ds, x, rng, kind, a, b, ang=None, t_sigma=0.02, info=None):
    """a pair prior near the entities' relative pose at x: its residual rotation is `ang` (default ~0.02 rad), its translation residual ~t_sigma"""
    xa, xb = pose_of(ds, x, kind, a), pose_of(ds, x, kind, b)
    Ra, Rb = rodrigues(xa[:3]), rodrigues(xb[:3])
    ang = 0.02 * (1 + rng.random()) if ang is None else ang
    Rrel = Ra.T @ Rb @ rodrigues(ang * unit(rng)).T   # R_rel^T R_ab = Exp(ang u)
    xrel = np.r_[so3_log(Rrel), Ra.T @ (xb[3:] - xa[3:]) + t_sigma * rng.standard_normal(3)]
    return (kind, a, b, xrel, random_spd(rng) if info is None else info)


# ---- 1. e and the cost ----
def rotation_case(kind):
    """g2_small with large entity rotations and pairs whose residual rotations run from 1e-9 to 2.5 rad"""
    ds, _ = load_golden("g2_small")
    rng = np.random.default_rng(11 if kind == "camera" else 12)
    fc, fm = free_entities(ds)
    x = ds.x_full.copy()
    for k, ents in (("camera", fc), ("marker", fm)):
        for i in ents:
            c = slot_col(ds, k, i)
            x[c:c + 3] = unit(rng) * rng.uniform(0.1, 2.0)
    if kind == "camera":
        ends = [(fc[0], fc[1]), (ds.root_cam, fc[0]), (fc[1], ds.root_cam)]
    else:
        ends = [(fm[0], fm[1]), (fm[2], fm[1]), (fm[2], fm[3]), (ds.root_marker, fm[4]), (fm[5], fm[4]), (fm[6], fm[0]), (fm[3], fm[6])]
    angles = [1e-9, 2.5, 1e-3, 0.5, 2.0, 1e-6, 1.0]
    return ds, x, [make_pair(ds, x, rng, kind, a, b, ang=angles[n % len(angles)], t_sigma=0.05) for n, (a, b) in enumerate(ends)]


@pytest.mark.parametrize("kind", ["camera", "marker"])
def test_pair_residuals_and_cost_match_numpy(kind):
    ds, x, pairs = rotation_case(kind)
    with Problem(ds, pair_priors=pairs) as p:
        assert aar.lib().aar_problem_num_pair_priors(p.handle) == len(pairs) and aar.lib().aar_problem_num_priors(p.handle) == 0
        e, cost = p.eval_pair_priors(x)
    ref = pair_residuals(ds, x, pairs)
    angles = np.linalg.norm(ref[:, :3], axis=1)
    assert angles.max() > 2.4 and angles.min() < 1e-8
    print("pair e: max abs error %.3e" % np.abs(e - ref).max())
    assert np.abs(e - ref).max() < 1e-12, np.abs(e - ref).max()
    cref = sum(r @ q[4] @ r for r, q in zip(ref, pairs))
    assert abs(cost - cref) <= 1e-12 * cref, (cost, cref)


# ---- 2. the blocks the pairs add to the normal equations ----
def block_case(name):
    """(fixture, pair ends as (kind, a, b) builder, keyword arguments both problems get, absolute priors both problems get)"""
    ds, _ = load_golden({"chain": "g1_cfg2", "many_pairs": "g1_cfg3_cut"}.get(name, "g2_small"))
    fc, fm = free_entities(ds)
    kw, spec = {}, []
    if name == "orientations":   # a < b and a > b, cameras and markers
        spec = [("camera", fc[0], fc[1]), ("marker", fm[0], fm[1]), ("marker", fm[3], fm[2]), ("marker", fm[5], fm[1])]
    elif name == "camera_high_first":
        spec = [("camera", fc[1], fc[0])]
    elif name == "star":   # four pairs on one marker, the centre as a and as b, lower and higher than its partners
        spec = [("marker", fm[3], fm[0]), ("marker", fm[1], fm[3]), ("marker", fm[3], fm[5]), ("marker", fm[6], fm[3])]
    elif name == "chain":   # every free marker and camera of g1_cfg2 in one chain each
        spec = [("marker", fm[i], fm[i + 1]) for i in range(len(fm) - 1)] + [("camera", fc[i + 1], fc[i]) for i in range(len(fc) - 1)]
    elif name == "root_end":
        spec = [("marker", ds.root_marker, fm[2]), ("camera", fc[1], ds.root_cam), ("marker", fm[2], fm[4])]
    elif name == "fixed_end":   # a caller-fixed end: its rows, its diagonal block and the cross block stay the twin's
        spec = [("marker", fm[1], fm[2]), ("marker", fm[3], fm[1]), ("camera", fc[0], fc[1])]
        kw = dict(fixed_markers=[fm[1]], fixed_cams=[fc[1]])
    elif name == "with_absolute_prior":
        spec = [("marker", fm[0], fm[1]), ("marker", fm[2], fm[0]), ("camera", fc[0], fc[1])]
    elif name == "many_pairs":   # more pairs than the kernel keeps in LDS (128): its instance on the global workspace; up to eight pairs an entity
        spec = [("marker", fm[i], fm[j]) if (i + j) % 2 else ("marker", fm[j], fm[i]) for i in range(len(fm)) for j in range(i + 1, min(i + 5, len(fm)))]
        assert len(spec) > 128
    return ds, spec, kw


BLOCK_CASES = ["orientations", "camera_high_first", "star", "chain", "root_end", "fixed_end", "with_absolute_prior", "many_pairs"]


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_normal_equation_blocks_match_the_restatement(name):
    ds, spec, kw = block_case(name)
    rng = np.random.default_rng(20 + BLOCK_CASES.index(name))
    x = ds.x_full
    fc, fm = free_entities(ds)
    if name == "with_absolute_prior":
        c = slot_col(ds, "marker", fm[0])
        kw["priors"] = [("marker", fm[0], x[c:c + 6] + 0.01 * rng.standard_normal(6), random_spd(rng, 1e3)),
                        ("camera", fc[0], x[slot_col(ds, "camera", fc[0]):slot_col(ds, "camera", fc[0]) + 6] + 0.01, random_spd(rng, 1e3))]
    # (deterministic: two problems then give the same bits wherever they compute the same thing, so `array_equal` below means something)
    with Problem(ds, solver="direct", deterministic=True, **kw) as tw:
        Ht, Bt, sst = tw.eval_normal_equations(x)
    # information matrices at a thousandth of the data's own diagonal: H_c - H_twin then keeps ~13 digits of the pairs' blocks
    # (the subtraction's cancellation, eps |H_twin| / |H_pairs|, stays below the kernel's own rounding of those blocks)
    scale = 1e-3 * float(np.diag(Ht).max()) / 12.0
    pairs = [make_pair(ds, x, rng, k, a, b, info=random_spd(rng, scale)) for k, a, b in spec]
    with Problem(ds, solver="direct", deterministic=True, pair_priors=pairs, **kw) as p:
        Hc, Bc, ssc = p.eval_normal_equations(x)
        _, cost = p.eval_pair_priors(x)
    P = len(Bt)
    fixed = [("marker", m) for m in kw.get("fixed_markers", [])] + [("camera", c) for c in kw.get("fixed_cams", [])]
    Hp, Bp, cref, touched = pair_terms(ds, x, pairs, P, fixed=fixed)
    assert abs(cost - cref) <= 1e-12 * cref
    assert abs(ssc - (sst + cost)) <= 1e-12 * ssc   # sum_sq carries the pairs' cost
    dH, dB = Hc - Ht, Bc - Bt
    worst = 0.0
    hmask, bmask = np.ones((P, P), bool), np.ones(P, bool)
    assert touched
    for ci, cj in set(touched):
        blk = (slice(ci, ci + 6), slice(cj, cj + 6))
        worst = max(worst, rel(dH[blk], Hp[blk]))
        hmask[blk] = False
        if ci == cj:
            worst = max(worst, rel(dB[ci:ci + 6], Bp[ci:ci + 6]))
            bmask[ci:ci + 6] = False
    print("pair blocks %s: largest relative block error %.3e" % (name, worst))
    assert worst < BLOCK_BAR, (name, worst)
    # nothing else moved, the rows and columns of a fixed end included
    assert np.array_equal(Hc[hmask], Ht[hmask])
    assert np.array_equal(Bc[bmask], Bt[bmask])
    assert not Hp[hmask].any() and not Bp[bmask].any()
    for kind, i in fixed:
        c = slot_col(ds, kind, i)
        assert np.array_equal(Hc[c:c + 6], Ht[c:c + 6]) and np.array_equal(Hc[:, c:c + 6], Ht[:, c:c + 6]) and np.array_equal(Bc[c:c + 6], Bt[c:c + 6])


# ---- 3. the damped step ----
_STEP_REF = {}


def step_case(huber):
    """g1_cfg3_cut: a chain over the cameras, a star and a chain over the markers, one absolute prior; the twin's H, B once per Huber setting"""
    if huber not in _STEP_REF:
        ds, _ = load_golden("g1_cfg3_cut")
        rng = np.random.default_rng(30)
        x = ds.x_full
        fc, fm = free_entities(ds)
        spec = [("camera", fc[i], fc[i + 1]) for i in range(len(fc) - 1)] + [("camera", fc[2], ds.root_cam)]
        spec += [("marker", fm[0], m) for m in fm[1:8]] + [("marker", fm[i + 1], fm[i]) for i in range(8, len(fm) - 1)]
        pairs = [make_pair(ds, x, rng, k, a, b, info=random_spd(rng, 1e3)) for k, a, b in spec]
        c = slot_col(ds, "marker", fm[0])
        priors = [("marker", fm[0], x[c:c + 6] + 0.01 * rng.standard_normal(6), random_spd(rng, 1e3))]
        with Problem(ds, with_huber=huber, solver="direct") as tw:
            Ht, Bt, _ = tw.eval_normal_equations(x)
        P = len(Bt)
        Hp, Bp, _, _ = pair_terms(ds, x, pairs, P)
        Ha, Ba, _ = prior_terms(ds, x, priors, P)
        _STEP_REF[huber] = (ds, x, pairs, priors, Ht + Hp + Ha, Bt + Bp + Ba, float(np.diag(Ht).max()))
    return _STEP_REF[huber]


@pytest.mark.parametrize("solver,huber", [(s, h) for s in ("direct", "spcg", "pcg") for h in (False, True)])
def test_damped_step_with_pair_priors(solver, huber):
    ds, x, pairs, priors, H, B, dmax = step_case(huber)
    tol = 1e-8 if solver == "direct" else 1e-6   # (the bars of test_gpu_pose_priors.py: the direct chain, an iterative solve)
    with Problem(ds, with_huber=huber, solver=solver, pair_priors=pairs, priors=priors, pcg_eta=None if solver == "direct" else 1e-12) as p:
        for mu in (dmax * 1e-2, dmax * 1e-5):
            d = p.eval_damped_step(x, mu)
            ref = np.linalg.solve(H + mu * np.eye(len(B)), B)
            print("damped step %s huber=%d mu=%.2e: relative error %.3e" % (solver, huber, mu, rel(d, ref)))
            assert rel(d, ref) < tol, (solver, huber, mu, rel(d, ref))


# ---- 4. end to end: a pair with a root end is the absolute prior ----
def test_pair_with_root_end_solves_like_the_absolute_prior():
    ds, _ = load_golden("g1_cfg2")
    rng = np.random.default_rng(40)
    x0 = ds.x_full
    fc, fm = free_entities(ds)
    priors, pairs = [], []
    for kind, ents, root in (("camera", fc, ds.root_cam), ("marker", fm, ds.root_marker)):
        for n, i in enumerate(ents):
            c = slot_col(ds, kind, i)
            xp = x0[c:c + 6] + np.r_[0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)]
            info = random_spd(rng, 1e2)
            priors.append((kind, i, xp, info))
            pairs.append((kind, root, i, xp, info))
    with Problem(ds, solver="direct", deterministic=True, priors=priors) as p:
        xa, ra = p.lm_solve(x0)
    with Problem(ds, solver="direct", deterministic=True, pair_priors=pairs) as p:
        xb, rb = p.lm_solve(x0)
    print("root-end pairs vs absolute priors: %d / %d LM steps, max |dx| %.3e" % (ra["iterations"], rb["iterations"], np.abs(xa - xb).max()))
    assert ra["iterations"] == rb["iterations"] and ra["iterations"] > 3
    assert np.abs(xa - xb).max() < 1e-9, np.abs(xa - xb).max()


# ---- 5. limits of the strength ----
def test_zero_information_is_bit_identical_in_deterministic_mode():
    ds, _ = load_golden("g1_cfg2")
    rng = np.random.default_rng(50)
    fc, fm = free_entities(ds)
    x0 = ds.x_full
    spec = [("marker", fm[0], m) for m in fm[1:]] + [("camera", fc[1], fc[0]), ("camera", ds.root_cam, fc[2])]
    pairs = [make_pair(ds, x0, rng, k, a, b, ang=0.3, info=np.zeros((6, 6))) for k, a, b in spec]
    with Problem(ds, solver="direct", deterministic=True) as p:
        xa, ra = p.lm_solve(x0)
    with Problem(ds, solver="direct", deterministic=True, pair_priors=pairs) as p:
        xb, rb = p.lm_solve(x0)
        _, cost = p.eval_pair_priors(x0)
    assert cost == 0.0
    assert np.array_equal(xa, xb)
    assert [t["err"] for t in ra["trace"]] == [t["err"] for t in rb["trace"]]


def test_stiff_marker_star_holds_the_layout():
    ds, _ = load_golden("g1_cfg2")
    fc, fm = free_entities(ds)
    prm = aar.lm_default_params(min_error=0.0, min_step_error_diff=0.0, min_average_step_error_diff=0.0, max_iters=400)
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64) as p:
        xs, _ = p.lm_solve(ds.x_full, params=prm)
    # the solved layout as a star on the first free marker, every arm moved by 1 mm, sigma 1e-6 (rad, m)
    pairs = []
    for n, m in enumerate(fm[1:]):
        xr = aar.relative_pose(pose_of(ds, xs, "marker", fm[0]), pose_of(ds, xs, "marker", m))
        xr[3 + n % 3] += 1e-3
        pairs.append(("marker", fm[0], m, xr, np.eye(6) / 1e-6 ** 2))
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64, pair_priors=pairs) as p:
        x, _ = p.lm_solve(xs, params=prm)
        e_dev, _ = p.eval_pair_priors(x)
    e = pair_residuals(ds, x, pairs)
    print("stiff star: largest |e| %.3e (before the solve %.3e)" % (np.abs(e).max(), np.abs(pair_residuals(ds, xs, pairs)).max()))
    assert np.abs(pair_residuals(ds, xs, pairs)).max() > 0.9e-3
    assert np.abs(e).max() < 1e-5, np.abs(e).max()
    assert np.abs(e_dev - e).max() < 1e-12


# ---- 7. two runs, the same bits ----
def test_two_runs_give_the_same_bits():
    ds, x, pairs, priors, _, _, dmax = step_case(False)
    out = []
    for _ in range(2):
        with Problem(ds, solver="direct", deterministic=True, pair_priors=pairs, priors=priors) as p:
            e1, c1 = p.eval_pair_priors(x)
            e2, c2 = p.eval_pair_priors(x)
            assert np.array_equal(e1, e2) and c1 == c2
            H, B, ss = p.eval_normal_equations(x)
            H2, B2, ss2 = p.eval_normal_equations(x)
            assert np.array_equal(H, H2) and np.array_equal(B, B2) and ss == ss2
            out.append((e1, c1, H, B, ss, p.eval_damped_step(x, dmax * 1e-3)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 8. covariance ----
def test_covariance_with_pair_priors():
    ds, _ = load_golden("g1_cfg2")
    rng = np.random.default_rng(80)
    x = ds.x_full
    fc, fm = free_entities(ds)
    spec = [("marker", fm[0], m) for m in fm[1:5]] + [("marker", fm[i + 1], fm[i]) for i in range(5, len(fm) - 1)] + [("camera", fc[0], fc[1]), ("camera", fc[2], fc[1])]
    pairs = [make_pair(ds, x, rng, k, a, b, info=random_spd(rng, 1e2)) for k, a, b in spec]
    with Problem(ds, solver="direct") as tw, Problem(ds, solver="direct", pair_priors=pairs, fixed_cams=[fc[0]]) as p:
        Ht, _, _ = tw.eval_normal_equations(x)
        cv = p.covariance(x, dense=True, frames=False)
    P = Ht.shape[0]
    Hp, _, _, _ = pair_terms(ds, x, pairs, P, fixed=[("camera", fc[0])])
    H = Ht + Hp
    held = np.zeros(P, bool)
    c = slot_col(ds, "camera", fc[0])
    held[c:c + 6] = True
    pe = 6 * (ds.num_cams - 1 + ds.num_markers - 1)
    live = ~held
    Hi = np.full((P, P), np.nan)
    Hi[np.ix_(live, live)] = np.linalg.inv(H[np.ix_(live, live)])
    ref = Hi[:pe, :pe]
    np.testing.assert_array_equal(np.isnan(cv.entity_cov), np.isnan(ref))
    m = ~np.isnan(ref)
    err = np.abs(cv.entity_cov[m] - ref[m]).max() / np.abs(ref[m]).max()
    print("covariance with pair priors: relative error %.3e" % err)
    assert err < 1e-7, err


# ---- 9. two in-process ranks ----
def test_two_ranks_match_one():
    ds, x, pairs, priors, _, _, dmax = step_case(False)
    mu = dmax * 1e-3
    kw = dict(solver="direct", deterministic=True, pair_priors=pairs, priors=priors)
    with Problem(ds, **kw) as p:
        e1, c1 = p.eval_pair_priors(x)
        d1 = p.eval_damped_step(x, mu)
    world = 2
    group = aar.LocalGroup(world)
    out, err = [None] * world, []

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with Problem(ds, comm=comm, **kw) as p:
                d = p.eval_damped_step(x, mu)
                out[r] = (p.eval_pair_priors(x), d)
        except Exception as ex:   # pragma: no cover - reported below
            err.append(ex)
        finally:
            comm.close()

    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    group.close()
    assert not err, err
    for (e, c), d in out:
        assert np.array_equal(e, e1) and c == c1
        print("two ranks: damped step relative difference to one GPU %.3e" % rel(d, d1))
        assert rel(d, d1) < 1e-9, rel(d, d1)
