"""Per-entity fixing and pose priors on the device.  Every reference is computed independently: the normal equations
of a TWIN problem without constraints (aar_eval_normal_equations at mu = 0) plus a numpy restatement of the prior terms."""
import os
import subprocess
import threading

import numpy as np
import pytest

import aar
from aar import Problem
from conftest import PKG, load_golden

pytestmark = pytest.mark.gpu


# ---- numpy restatement of the prior (include/aar.h): tests/reduced_system.py ----
from reduced_system import prior_e, prior_terms, rodrigues, slot_col, so3_log  # noqa: E402


def free_entities(ds):
    return [c for c in range(ds.num_cams) if c != ds.root_cam], [m for m in range(ds.num_markers) if m != ds.root_marker]


def random_spd(rng, scale=1.0):
    A = rng.standard_normal((6, 6))
    return scale * (A @ A.T + 6 * np.eye(6))


def random_priors(ds, x, rng, scale=1e3, rot_sigma=0.02, t_sigma=0.01):
    fc, fm = free_entities(ds)
    pr = []
    for kind, ents in (("camera", fc), ("marker", fm)):
        for i in ents:
            c = slot_col(ds, kind, i)
            xp = x[c:c + 6] + np.r_[rot_sigma * rng.standard_normal(3), t_sigma * rng.standard_normal(3)]
            pr.append((kind, i, xp, random_spd(rng, scale)))
    return pr


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- 1. the prior terms ----
def test_prior_residuals_and_cost_match_numpy_at_large_rotations():
    ds, _ = load_golden("g2_small")
    rng = np.random.default_rng(1)
    fc, fm = free_entities(ds)
    x = ds.x_full.copy()
    priors = []
    for n, (kind, i) in enumerate([("camera", c) for c in fc] + [("marker", m) for m in fm]):
        col = slot_col(ds, kind, i)
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        x[col:col + 3] = ax * rng.uniform(0.1, 2.0)
        # relative rotations from 1e-9 rad to 2.5 rad
        rel_ang = [1e-9, 1e-3, 0.5, 2.0, 2.5][n % 5]
        R = rodrigues(x[col:col + 3]) @ rodrigues(-rel_ang * ax[[1, 2, 0]] / np.linalg.norm(ax[[1, 2, 0]]))
        w = so3_log(R)
        priors.append((kind, i, np.r_[w, x[col + 3:col + 6] + rng.standard_normal(3) * 0.05], random_spd(rng)))
    with Problem(ds, priors=priors) as p:
        assert aar.lib().aar_problem_num_priors(p.handle) == len(priors)
        e, cost = p.eval_priors(x)
    ref = np.array([prior_e(x[slot_col(ds, k, i):slot_col(ds, k, i) + 6], xp) for k, i, xp, _ in priors])
    assert np.abs(e - ref).max() < 1e-12, np.abs(e - ref).max()
    cref = sum(r @ info @ r for r, (_, _, _, info) in zip(ref, priors))
    assert abs(cost - cref) <= 1e-12 * cref
    angles = np.linalg.norm(ref[:, :3], axis=1)
    assert angles.max() > 2.4 and angles.min() < 1e-8


def test_prior_hessian_and_gradient_match_central_differences():
    ds, _ = load_golden("g2_small")
    rng = np.random.default_rng(2)
    x = ds.x_full.copy()
    priors = random_priors(ds, x, rng, scale=10.0, rot_sigma=0.8, t_sigma=0.2)
    with Problem(ds) as tw, Problem(ds, priors=priors) as p:
        Ht, Bt, sst = tw.eval_normal_equations(x)
        Hc, Bc, ssc = p.eval_normal_equations(x)
        _, cost = p.eval_priors(x)
    assert abs(ssc - (sst + cost)) <= 1e-12 * ssc   # sum_sq carries the priors' cost
    for kind, i, xp, info in priors:
        c = slot_col(ds, kind, i)
        x6 = x[c:c + 6]
        Jn = np.zeros((6, 6))
        for k in range(6):
            h = 1e-6
            d = np.zeros(6)
            d[k] = h
            Jn[:, k] = (prior_e(x6 + d, xp) - prior_e(x6 - d, xp)) / (2 * h)
        e = prior_e(x6, xp)
        Hn, gn = Jn.T @ info @ Jn, -Jn.T @ info @ e
        dH = Hc[c:c + 6, c:c + 6] - Ht[c:c + 6, c:c + 6]
        dB = Bc[c:c + 6] - Bt[c:c + 6]
        assert rel(dH, Hn) < 1e-6, (kind, i, rel(dH, Hn))
        assert rel(dB, gn) < 1e-6, (kind, i, rel(dB, gn))
    # nothing else moved
    mask = np.ones(len(Bt), bool)
    for kind, i, _, _ in priors:
        c = slot_col(ds, kind, i)
        mask[c:c + 6] = False
    assert np.array_equal(Bc[mask], Bt[mask])


# ---- 2. the damped step with priors ----
@pytest.mark.parametrize("name,huber", [("g1_cfg2", False), ("g2_small", False), ("g1_cfg3_cut", False), ("g1_cfg2", True)])
def test_damped_step_with_priors(name, huber):
    ds, _ = load_golden(name)
    rng = np.random.default_rng(3)
    x = ds.x_full
    priors = random_priors(ds, x, rng)
    with Problem(ds, with_huber=huber, solver="direct") as tw, Problem(ds, with_huber=huber, solver="direct", priors=priors) as p:
        Ht, Bt, _ = tw.eval_normal_equations(x)
        Hp, Bp, _ = prior_terms(ds, x, priors, len(Bt))
        for mu in (float(np.diag(Ht).max()) * 1e-2, float(np.diag(Ht).max()) * 1e-5):
            d = p.eval_damped_step(x, mu)
            ref = np.linalg.solve(Ht + mu * np.eye(len(Bt)) + Hp, Bt + Bp)
            assert rel(d, ref) < 1e-8, (name, mu, rel(d, ref))


# ---- 3. the damped step with fixed indices ----
@pytest.mark.parametrize("solver", ["direct", "spcg"])
def test_damped_step_with_fixed_indices(solver):
    ds, _ = load_golden("g1_cfg3_cut")
    fc, fm = free_entities(ds)
    fix_c, fix_m = fc[:2], fm[1:4]
    x = ds.x_full
    with Problem(ds, solver="direct") as tw, Problem(ds, solver=solver, fixed_cams=fix_c + [ds.root_cam], fixed_markers=fix_m,
                                                  pcg_eta=1e-12 if solver == "spcg" else None) as p:
        Ht, Bt, _ = tw.eval_normal_equations(x)
        assert p.num_vars == tw.num_vars
        mu = float(np.diag(Ht).max()) * 1e-3
        d = p.eval_damped_step(x, mu)
    held = np.zeros(len(Bt), bool)
    for c in fix_c:
        held[slot_col(ds, "camera", c):slot_col(ds, "camera", c) + 6] = True
    for m in fix_m:
        held[slot_col(ds, "marker", m):slot_col(ds, "marker", m) + 6] = True
    assert np.all(d[held] == 0.0)
    fr = ~held
    ref = np.linalg.solve(Ht[np.ix_(fr, fr)] + mu * np.eye(fr.sum()), Bt[fr])
    tol = 1e-8 if solver == "direct" else 1e-6   # (SPCG: an iterative solve)
    assert rel(d[fr], ref) < tol, rel(d[fr], ref)


# ---- 4. rig extension ----
def cam_block(x, ds, c):
    return x[slot_col(ds, "camera", c):slot_col(ds, "camera", c) + 6]


def test_rig_extension_config3():
    ds = aar.synth(3)
    assert ds.num_cams == 8
    # (every solve to a tight stopping rule, with fp64 residuals whose error function is smooth enough for it: the reference's own rule stops
    #  wherever its average error drop falls under 1e-3, and residuals rounded to float leave a noise floor in the error)
    prm = aar.lm_default_params(min_error=0.0, min_step_error_diff=0.0, min_average_step_error_diff=1e-12, max_iters=300)
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64) as p:
        x_full, rep_full = p.lm_solve(ds.x_full, params=prm)
        rmse_full, _ = p.reproj_stats(x_full)
    rng = np.random.default_rng(4)
    x0 = x_full.copy()
    new_cam = 7 if ds.root_cam != 7 else 6
    c = slot_col(ds, "camera", new_cam)
    x0[c:c + 6] += np.r_[0.02 * rng.standard_normal(3), 0.02 * rng.standard_normal(3)]
    m0 = 6 * (ds.num_cams - 1)
    x0[m0:m0 + 6 * (ds.num_markers - 1)] += 0.005 * rng.standard_normal(6 * (ds.num_markers - 1))
    fixed = [k for k in range(8) if k != new_cam]
    finals = {}
    for solver in ("direct", "spcg", "pcg", "auto"):
        with Problem(ds, solver=solver, fixed_cams=fixed, residual_mode=aar.RES_F64, pcg_eta=None if solver == "direct" else 1e-8) as p:
            x, rep = p.lm_solve(x0, params=prm)
            rmse, _ = p.reproj_stats(x)
        for k in fixed:
            if k != ds.root_cam:
                assert np.array_equal(cam_block(x, ds, k), cam_block(x0, ds, k)), (solver, k)
        assert np.abs(cam_block(x, ds, new_cam) - cam_block(x_full, ds, new_cam)).max() < 1e-4, solver
        assert abs(rmse - rmse_full) < 1e-6, (solver, rmse, rmse_full)
        finals[solver] = x
    for s in ("spcg", "pcg", "auto"):
        assert np.abs(finals[s][:m0 + 6 * (ds.num_markers - 1)] - finals["direct"][:m0 + 6 * (ds.num_markers - 1)]).max() < 1e-5, s


# ---- 5. limits of the prior strength ----
def test_stiff_prior_is_fixing():
    ds, _ = load_golden("g1_cfg2")
    fc, fm = free_entities(ds)
    x0 = ds.x_full
    c = slot_col(ds, "camera", fc[0])
    prm = aar.lm_default_params(min_error=0.0, min_step_error_diff=0.0, min_average_step_error_diff=0.0, max_iters=400)
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64, fixed_cams=[fc[0]]) as p:
        xf, _ = p.lm_solve(x0, params=prm)
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64, priors=[("camera", fc[0], x0[c:c + 6], 1e12 * np.eye(6))]) as p:
        xs, _ = p.lm_solve(x0, params=prm)
    assert np.abs(xs - xf).max() < 1e-6, np.abs(xs - xf).max()


def test_zero_priors_are_bit_identical_in_deterministic_mode():
    ds, _ = load_golden("g1_cfg2")
    fc, fm = free_entities(ds)
    x0 = ds.x_full
    priors = [(k, i, x0[slot_col(ds, k, i):slot_col(ds, k, i) + 6] + 0.1, np.zeros((6, 6)))
              for k, ents in (("camera", fc), ("marker", fm)) for i in ents]
    with Problem(ds, solver="direct", deterministic=True) as p:
        xa, ra = p.lm_solve(x0)
    with Problem(ds, solver="direct", deterministic=True, priors=priors) as p:
        xb, rb = p.lm_solve(x0)
    assert np.array_equal(xa, xb)
    assert [t["err"] for t in ra["trace"]] == [t["err"] for t in rb["trace"]]


def test_empty_constraints_are_create_ex():
    ds = aar.synth(3)
    prm = aar.lm_default_params(max_iters=15, min_error=0.0, min_step_error_diff=0.0, min_average_step_error_diff=0.0)
    with Problem(ds, solver="direct", deterministic=True) as p:
        xa, ra = p.lm_solve(ds.x_full, params=prm)
    with Problem(ds, solver="direct", deterministic=True, constrained=True) as p:
        xb, rb = p.lm_solve(ds.x_full, params=prm)
    assert ra["iterations"] == rb["iterations"] == 15
    assert np.array_equal(xa, xb)
    for a, b in zip(ra["trace"], rb["trace"]):
        assert a == b


# ---- 6. optimality ----
def test_converged_point_is_stationary_for_the_total_cost():
    ds, _ = load_golden("g1_cfg2")
    rng = np.random.default_rng(6)
    x0 = ds.x_full
    priors = random_priors(ds, x0, rng, scale=1e2, rot_sigma=0.01, t_sigma=0.01)
    fc, _ = free_entities(ds)
    prm = aar.lm_default_params(min_error=0.0, min_step_error_diff=0.0, min_average_step_error_diff=1e-12, max_iters=200)
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64, priors=priors[1:], fixed_cams=[fc[0]]) as p:
        x, _ = p.lm_solve(x0, params=prm)
    with Problem(ds, solver="direct", residual_mode=aar.RES_F64) as tw:
        _, B0, _ = tw.eval_normal_equations(x0)
        _, B1, _ = tw.eval_normal_equations(x)
    P = len(B0)
    _, Bp0, _ = prior_terms(ds, x0, priors[1:], P)
    _, Bp1, _ = prior_terms(ds, x, priors[1:], P)
    free = np.ones(P, bool)
    c = slot_col(ds, "camera", fc[0])
    free[c:c + 6] = False
    g0, g1 = (B0 + Bp0)[free], (B1 + Bp1)[free]
    assert np.linalg.norm(g1) < 1e-6 * np.linalg.norm(g0), (np.linalg.norm(g1), np.linalg.norm(g0))


# ---- 7. covariance ----
def test_covariance_with_priors_and_fixed_indices():
    ds, _ = load_golden("g1_cfg2")
    rng = np.random.default_rng(7)
    x = ds.x_full
    fc, fm = free_entities(ds)
    priors = random_priors(ds, x, rng, scale=1e2)
    priors = [q for q in priors if not (q[0] == "camera" and q[1] == fc[0])]
    with Problem(ds, solver="direct") as tw, Problem(ds, solver="direct", priors=priors, fixed_cams=[fc[0]]) as p:
        Ht, _, _ = tw.eval_normal_equations(x)
        cv = p.covariance(x, dense=True, frames=False)
    P = Ht.shape[0]
    Hp, _, _ = prior_terms(ds, x, priors, P)
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
    assert np.abs(cv.entity_cov[m] - ref[m]).max() / np.abs(ref[m]).max() < 1e-7


# ---- 8. multi-rank ----
def _ranks(world, ds, x0, kw):
    group = aar.LocalGroup(world)
    out = [None] * world
    err = []

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with Problem(ds, comm=comm, **kw) as p:
                out[r] = p.lm_solve(x0)[0]
        except Exception as e:   # pragma: no cover - reported below
            err.append(e)
        finally:
            comm.close()

    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    group.close()
    assert not err, err
    return out


def test_multi_rank_matches_one_rank():
    solver = "direct"
    ds = aar.synth(4)
    rng = np.random.default_rng(8)
    x0 = ds.x_full
    fc, fm = free_entities(ds)
    priors = [q for q in random_priors(ds, x0, rng, scale=1e2) if not (q[0] == "camera" and q[1] == fc[0]) and not (q[0] == "marker" and q[1] == fm[0])]
    kw = dict(solver=solver, deterministic=True, priors=priors, fixed_cams=[fc[0]], fixed_markers=[fm[0]])
    with Problem(ds, **kw) as p:
        x1, _ = p.lm_solve(x0)
    for world in (2, 4):
        xs = _ranks(world, ds, x0, kw)
        for x in xs:
            assert np.abs(x - x1).max() < 1e-9, (world, np.abs(x - x1).max())


# ---- 9. CLI ----
def test_cli_fix_cams_and_prior_solution(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "s2")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, timeout=120).returncode == 0
    ini = aar.solution_read(os.path.join(folder, "initial.solution"))
    fc, fm = free_entities(ini)
    fix_id = int(ini.cam_ids[fc[0]])
    r = subprocess.run([exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-fix-cams", str(fix_id), "-prior-solution",
                        os.path.join(folder, "initial.solution"), "-prior-sigma-deg", "2", "-prior-sigma-m", "0.05"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "constraints: 1 fixed camera(s), 0 fixed marker(s), %d pose prior(s)" % (len(fc) - 1 + len(fm)) in r.stdout
    assert "final error: reprojection" in r.stdout and "+ prior" in r.stdout
    fin = aar.solution_read(os.path.join(folder, "final.solution"))
    c = slot_col(ini, "camera", fc[0])
    # the fixed camera comes back as it went in (up to the mapper's pose -> 4x4 -> pose round trip of the file writer)
    assert np.abs(fin.x_full[c:c + 6] - ini.x_full[c:c + 6]).max() < 1e-12
    # ... and the free ones moved, but the priors held them near the initial solution
    c2 = slot_col(ini, "camera", fc[1])
    assert np.abs(fin.x_full[c2:c2 + 6] - ini.x_full[c2:c2 + 6]).max() > 1e-7
