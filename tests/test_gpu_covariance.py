"""aar_problem_covariance on the device against numpy's inverse of the dense J^T J, through fixed groups, intrinsics, every
solver, unobserved entities, sharded problems, and a Monte Carlo check that the numbers mean what they say."""
import threading
import time

import numpy as np
import pytest

import aar
from aar import Problem
from conftest import load_golden

pytestmark = pytest.mark.gpu


def dense_inverse(H):
    """inv(H) over the rows / columns that are not identically zero; NaN elsewhere"""
    live = np.abs(H).sum(axis=1) != 0
    out = np.full_like(H, np.nan)
    out[np.ix_(live, live)] = np.linalg.inv(H[np.ix_(live, live)])
    return out


def block_err(a, b, scale):
    """relative Frobenius difference of one block, NaN patterns equal"""
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    m = ~np.isnan(b)
    if not m.any():
        return 0.0
    return np.linalg.norm(a[m] - b[m]) / scale


def compare(p, x, tol=1e-7, dense=True):
    """the device covariance of problem p at x against numpy; returns (worst block error, covariance)"""
    H, _, ss = p.eval_normal_equations(x)
    Hi = dense_inverse(H)
    cv = p.covariance(x, dense=dense)
    sizes = p.entity_block_sizes()
    pe = sum(sizes)
    nF = p.ds.num_frames if p.optimize[2] else 0
    # z order: [cameras | markers] | frames | intrinsics -> entity columns skip the frames
    f0 = (6 * (p.ds.num_cams - 1) if p.optimize[0] else 0) + (6 * (p.ds.num_markers - 1) if p.optimize[1] else 0)
    ecols = np.r_[0:f0, f0 + 6 * nF:p.num_vars]
    He = Hi[np.ix_(ecols, ecols)]
    assert He.shape == (pe, pe)
    starts = np.cumsum([0] + sizes)
    dscale = [np.linalg.norm(np.nan_to_num(He[s:s + b, s:s + b])) or 1.0 for s, b in zip(starts, sizes)]
    worst = 0.0
    for k, (s, b) in enumerate(zip(starts, sizes)):
        worst = max(worst, block_err(cv.entity_diag[k], He[s:s + b, s:s + b], dscale[k]))
    if dense:
        for i, (si, bi) in enumerate(zip(starts, sizes)):
            for j, (sj, bj) in enumerate(zip(starts, sizes)):
                worst = max(worst, block_err(cv.entity_cov[si:si + bi, sj:sj + bj], He[si:si + bi, sj:sj + bj], np.sqrt(dscale[i] * dscale[j])))
    if nF:
        for f in range(nF):
            ref = Hi[f0 + 6 * f:f0 + 6 * f + 6, f0 + 6 * f:f0 + 6 * f + 6]
            worst = max(worst, block_err(cv.frames[f], ref, np.linalg.norm(np.nan_to_num(ref)) or 1.0))
        assert cv.frames_written == nF
    else:
        assert cv.frames is None and cv.frames_written == 0
    assert worst <= tol, worst
    assert cv.num_vars == p.num_vars and cv.num_residuals == 8 * p.ds.num_obs
    np.testing.assert_allclose(cv.sum_sq, ss, rtol=1e-12)
    np.testing.assert_allclose(cv.sigma2, ss / (8 * p.ds.num_obs - p.num_vars), rtol=1e-12)
    assert 0 < cv.min_pivot <= cv.max_pivot
    return worst, cv


@pytest.mark.parametrize("name", ["g1_cfg2", "g1_cfg2_huber", "g2_small", "g1_cfg3_cut"])
def test_against_dense_inverse(name):
    ds, _ = load_golden(name)
    with Problem(ds, with_huber=name.endswith("huber"), solver="direct") as p:
        worst, cv = compare(p, ds.x_full)
        print("%s: worst block error %.2e, pivots %.3e .. %.3e (ratio %.2e)" % (name, worst, cv.min_pivot, cv.max_pivot, cv.max_pivot / cv.min_pivot))


def test_config3_full_size():
    ds = aar.synth(3)
    with Problem(ds, solver="direct") as p:
        assert p.num_vars == 3276
        worst, cv = compare(p, ds.x_full)
        print("config 3: worst block error %.2e, pivot ratio %.2e" % (worst, cv.max_pivot / cv.min_pivot))


def test_intrinsics_distortion_rows_are_nan():
    ds, _ = load_golden("g1_cfg2_intr")
    with Problem(ds, intrinsics=True, solver="direct") as p:
        x0 = p.x_with_intrinsics(ds.x_full)
        _, cv = compare(p, x0)
        for blk in cv.entity_diag[-ds.num_cams:]:
            assert blk.shape == (9, 9)
            assert np.isnan(blk[4:, :]).all() and np.isnan(blk[:, 4:]).all() and np.isfinite(blk[:4, :4]).all()


@pytest.mark.parametrize("opt", [(0, 1, 1), (1, 0, 1), (1, 1, 0)])
def test_fixed_groups(opt):
    ds, _ = load_golden("g1_cfg2")
    with Problem(ds, optimize=opt, solver="direct") as p:
        _, cv = compare(p, ds.x_full)
        if not opt[2]:
            assert cv.frames is None and cv.frames_written == 0


def test_solver_independence():
    # deterministic problems (every fp64 sum in a fixed order): DIRECT, SPCG, PCG and AUTO give the same bits -- the call always takes
    # the direct chain.  Default problems leave the Schur complement to fp64 atomics, whose order changes from run to run: the
    # results then agree to rounding amplified by the conditioning (pivot ratio ~6e5 here), 1e-10 of each block's scale.
    ds, _ = load_golden("g1_cfg3_cut")
    for det in (True, False):
        res = {}
        for s in ("direct", "spcg", "pcg", "auto"):
            with Problem(ds, solver=s, deterministic=det) as p:
                res[s] = p.covariance(ds.x_full, dense=True)
        ref = res["direct"]
        for s, cv in res.items():
            if det:
                assert np.array_equal(cv.entity_cov, ref.entity_cov, equal_nan=True), s
                assert np.array_equal(cv.frames, ref.frames), s
                assert cv.sigma2 == ref.sigma2 and cv.min_pivot == ref.min_pivot, s
            else:
                np.testing.assert_array_equal(np.isnan(cv.entity_cov), np.isnan(ref.entity_cov))
                d = np.sqrt(np.abs(np.nan_to_num(np.diag(ref.entity_cov))))
                assert (np.nan_to_num(np.abs(cv.entity_cov - ref.entity_cov)) <= 1e-10 * np.outer(d, d)).all(), s
                fs = np.linalg.norm(ref.frames, axis=(1, 2))
                assert (np.linalg.norm(cv.frames - ref.frames, axis=(1, 2)) <= 1e-10 * fs).all(), s
                np.testing.assert_allclose(cv.sigma2, ref.sigma2, rtol=1e-13)


def _drop(ds, keep):
    """a copy of ds with only the observations in mask `keep`"""
    import copy
    d2 = copy.copy(ds)
    for k in ("obs_frame", "obs_cam", "obs_marker"):
        setattr(d2, k, np.ascontiguousarray(getattr(ds, k)[keep]))
    d2.obs_uv = np.ascontiguousarray(ds.obs_uv.reshape(-1, 8)[keep].reshape(-1))
    d2.num_obs = int(keep.sum())
    return d2


def test_unobserved_marker_and_empty_frame():
    ds, _ = load_golden("g1_cfg2")
    rm = ds.root_marker
    m_gone = (rm + 1) % ds.num_markers
    f_gone = 3
    keep = (ds.obs_marker != m_gone) & (ds.obs_frame != f_gone)
    d2 = _drop(ds, keep)
    with Problem(d2, solver="direct") as p:
        _, cv = compare(p, d2.x_full)
    ms = m_gone if m_gone < rm else m_gone - 1
    k = ds.num_cams - 1 + ms
    assert np.isnan(cv.entity_diag[k]).all()
    assert np.isnan(cv.frames[f_gone]).all()
    # (the values of every block are checked against numpy's inverse of this data set's J^T J by compare() above)
    with Problem(ds, solver="direct") as p:
        full = p.covariance(ds.x_full)
    others = [i for i in range(len(cv.entity_diag)) if i != k]
    assert all(np.array_equal(np.isnan(cv.entity_diag[i]), np.isnan(full.entity_diag[i])) for i in others)
    assert not np.isnan(full.entity_diag[k]).any()
    assert np.isfinite(np.delete(cv.frames, f_gone, axis=0)).all()


def _ranks(world, ds, x):
    group = aar.LocalGroup(world)
    out = [None] * world

    def body(r):
        comm = aar.Comm.local(group, r, 0)
        try:
            with Problem(ds, comm=comm, solver="direct") as p:
                out[r] = p.covariance(x, dense=False)
        except Exception as e:
            out[r] = e
        finally:
            comm.close()
    th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th), "a rank is stuck"
    group.close()
    for o in out:
        assert not isinstance(o, Exception), o
    return out


@pytest.mark.parametrize("world", [2, 4])
def test_multi_rank(world):
    ds = aar.synth(4)
    assert ds.num_frames == 2000
    with Problem(ds, solver="direct") as p:
        one = p.covariance(ds.x_full)
    out = _ranks(world, ds, ds.x_full)
    d0 = out[0].entity_diag_flat
    filled = np.zeros(ds.num_frames, dtype=int)
    for cv in out:
        assert np.array_equal(cv.entity_diag_flat, d0, equal_nan=True)   # identical bits on every rank
        np.testing.assert_allclose(cv.sigma2, one.sigma2, rtol=1e-12)
        fin = np.isfinite(cv.frames).all(axis=(1, 2))
        assert fin.sum() == cv.frames_written > 0
        filled += fin
        np.testing.assert_allclose(cv.frames[fin], one.frames[fin], rtol=1e-9, atol=1e-11 * np.nanmax(np.abs(one.frames)))
    assert (filled == 1).all()     # every frame written by exactly one rank
    # (the ranks' Schur terms are summed in another order than one GPU's atomics do: rounding, amplified by the conditioning)
    np.testing.assert_allclose(d0, one.entity_diag_flat, rtol=1e-9, atol=1e-11 * np.nanmax(np.abs(one.entity_diag_flat)))


def test_config5_full_size():
    ds = aar.synth(5)
    with Problem(ds) as p:
        p.covariance(ds.x_full, dense=False)   # (workspace allocation, code objects)
        t0 = time.perf_counter()
        cv = p.covariance(ds.x_full, dense=False)
        dt = time.perf_counter() - t0
    print("config 5: one covariance call %.2f ms (host copies of the outputs included), pivot ratio %.2e" % (dt * 1e3, cv.max_pivot / cv.min_pivot))
    seen = [b for b in cv.entity_diag if not np.isnan(b).all()]   # (markers no frame of the sequence sees are NaN blocks)
    assert len(seen) >= 0.9 * len(cv.entity_diag)
    for b in seen:
        assert np.isfinite(b).all()
        np.testing.assert_allclose(b, b.T, rtol=1e-9, atol=1e-12 * np.abs(b).max())
        assert np.linalg.eigvalsh(0.5 * (b + b.T)).min() > 0
    assert np.isfinite(cv.frames).all()
    fr = 0.5 * (cv.frames + cv.frames.transpose(0, 2, 1))
    assert (np.linalg.eigvalsh(fr).min(axis=1) > 0).all()


def test_monte_carlo_calibration():
    # 40 noisy realisations of config 2 solved to convergence: the predicted covariance sigma2 * Sigma whitens the actual error
    prm = aar.lm_default_params(max_iters=200, min_average_step_error_diff=0.0, min_step_error_diff=0.0, min_error=0.0)
    chi_e, chi_f, s2 = [], [], []
    for seed in range(40):
        ds = aar.synth(2, seed=20190221 + 1000 * seed)
        with Problem(ds, residual_mode=aar.RES_F64, solver="direct") as p:
            x = ds.x_full.copy()
            x, _ = p.lm_solve(x, params=prm)
            cv = p.covariance(x)
            sd_e = np.sqrt(cv.sigma2 * np.concatenate([np.diag(b) for b in cv.entity_diag]))
            sd_f = np.sqrt(cv.sigma2 * np.concatenate([np.diag(b) for b in cv.frames]))
            H, B, _ = p.eval_normal_equations(x)
            step = np.nan_to_num(dense_inverse(H)) @ B          # the Gauss-Newton step (rows of unobserved entities: none)
            ne = len(sd_e)
            # the solution is converged: one more Gauss-Newton step moves no coordinate by 1 % of its predicted sigma
            ok_e = ~np.isnan(sd_e)
            assert (np.abs(step[:ne][ok_e]) <= 1e-2 * sd_e[ok_e]).all() and (np.abs(step[ne:]) <= 1e-2 * sd_f).all()
            e = p.extract_z(x) - p.extract_z(ds.x_truth)
            for k, b in enumerate(cv.entity_diag):
                if np.isnan(b).any():
                    continue
                d = e[6 * k:6 * k + 6]
                chi_e.append(d @ np.linalg.solve(cv.sigma2 * b, d))
            for f in range(ds.num_frames):
                d = e[ne + 6 * f:ne + 6 * f + 6]
                chi_f.append(d @ np.linalg.solve(cv.sigma2 * cv.frames[f], d))
            s2.append(cv.sigma2)
    print("Monte Carlo: mean chi2 entities %.3f (%d blocks), frames %.3f (%d blocks), mean sigma2 %.4f"
          % (np.mean(chi_e), len(chi_e), np.mean(chi_f), len(chi_f), np.mean(s2)))
    assert 5.2 <= np.mean(chi_e) <= 6.8
    assert 5.6 <= np.mean(chi_f) <= 6.4
    assert abs(np.mean(s2) / 0.09 - 1) < 0.1


def test_find_solution_covariance_switch(tmp_path):
    # aar_find_solution -covariance (MultiCamMapper::compute_covariance + aar_covariance_write_yaml) writes final.covariance.yaml
    # beside final.solution; without the switch nothing else changes (fixed-order sums, so that two solves give the same bits)
    import os
    import subprocess
    from conftest import PKG
    from test_covariance_host import parse_cov_yaml
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")   # (one folder for both runs: the files record paths)
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    env = dict(os.environ, AAR_DETERMINISTIC="1")
    got = {}
    for flag in ([], ["-covariance"]):
        run = subprocess.run([exe, folder, "0.05", "x", "-from-initial", "-solver", "direct"] + flag, capture_output=True, text=True, timeout=300, env=env)
        assert run.returncode == 0, run.stderr
        assert os.path.exists(os.path.join(folder, "final.covariance.yaml")) == bool(flag)
        got[bool(flag)] = [open(os.path.join(folder, f), "rb").read() for f in ("final.solution", "final.solution.yaml")]
    assert got[False] == got[True]
    outs = {True: folder}
    y = parse_cov_yaml(os.path.join(outs[True], "final.covariance.yaml"))
    sol = aar.solution_read(os.path.join(outs[True], "final.solution"))
    assert set(y["cameras"]) == set(int(i) for i in sol.cam_ids) and len(y["object_poses"]) == sol.num_frames
    with Problem(sol, solver="direct") as p:
        cv = p.covariance(sol.x_full)
    np.testing.assert_allclose(y["sigma2"], cv.sigma2, rtol=1e-6)
    k = 0
    for c in range(sol.num_cams):
        blk = y["cameras"][int(sol.cam_ids[c])][2]
        if c == sol.root_cam:
            assert np.isnan(blk).all()
            continue
        np.testing.assert_allclose(blk, cv.sigma2 * cv.entity_diag[k], rtol=1e-6)
        k += 1
