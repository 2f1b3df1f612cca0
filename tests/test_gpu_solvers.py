"""The solvers of the damped normal equations behind aar_solver_options (include/aar.h) -- DIRECT (the reference's step to rounding,
libs/sparselevmarq.h:394-400), SPCG (CG on the explicit reduced system, csrc/spcg_kernels.hip), PCG (CG through the frame blocks,
csrc/pcg_kernels.hip), AUTO -- against each other, the CPU oracle and the compiled reference.  Needs a real MI355X.

Bars: at a tight forcing term an inexact solver's damped step IS the direct step (<= 1e-8 relative, fixed-order sums); with the library's DEFAULT options
(solver AUTO, default forcing terms) the LM run ends within 1e-4 px of the reference-faithful CPU run (north star), within 1e-6 px of the direct path, in as
many LM steps, and its final POSES -- as transforms: rotation-matrix entries and translations, tests/pose_metrics.py -- agree with the direct path's to
1e-6 (cameras) / 1e-5 (markers, frames) and with the reference-faithful CPU run's as closely as the direct path's own do (3e-4: what the analytic Jacobian
costs against the reference's central-difference float Jacobian; the reference's own last LM step still moves the poses by ~3e-3).
"""
import os
import threading

import numpy as np
import pytest

import aar
import oracle_lib as ol
from conftest import load_golden
from pose_metrics import pose_delta, pose_delta_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("name,kw", [("g1_cfg2", {}), ("g1_cfg3_cut", {}), ("g1_cfg3_cut", {"optimize": (False, True, True)}), ("g1_cfg3_cut", {"optimize": (True, False, True)}),
                                     ("g1_cfg2_intr", {"intrinsics": True}), ("g2_small", {})])
def test_spcg_damped_step_is_the_direct_step_at_a_tight_forcing_term(name, kw):
    # one to four tiles, gauge rows, switched-off groups, the intrinsics entities: the CG on the explicit reduced system converged to 1e-12 gives the
    # step of the dense LDL^T chain and of the oracle's sparse LDL^T.  Fixed-order sums (deterministic): the same S to the bit on both sides, so the
    # comparison sees the two SOLVES only, and the iteration count does not move with the order of fp64 atomics
    ds, g = load_golden(name)
    o = ol.Oracle(ds, **({"optimize": kw["optimize"]} if "optimize" in kw else {}), **({"intrinsics": True} if kw.get("intrinsics") else {}))
    with aar.Problem(ds, solver="direct", deterministic=True, **kw) as pd, aar.Problem(ds, solver="spcg", pcg_eta=1e-12, deterministic=True, **kw) as ps:
        x0 = pd.x_with_intrinsics(ds.x_full) if kw.get("intrinsics") else ds.x_full
        assert ps.solver_stats()["solver"] == "spcg" and pd.solver_stats()["solver"] == "direct"
        for mu in (1e2, 1e5, 1e8):
            dd, dsp = pd.eval_damped_step(x0, mu), ps.eval_damped_step(x0, mu)
            st = ps.solver_stats()
            # (1e-8 while the damping keeps the system's condition number below ~1e5; at mu = 1e2 it is ~1e7 and a residual of 1e-12 in the preconditioner's
            #  norm bounds the error by 1e-7 only: 1.3e-8 observed, the same on every run under fixed-order sums)
            assert _rel(dsp, dd) < (1e-8 if mu >= 1e5 else 1e-7), (mu, st)
            if not kw.get("intrinsics"):
                do = o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
                assert _rel(dsp, do) < 1e-7, mu
        st = ps.solver_stats()
        assert st["solves"] >= 3 and st["total_iterations"] > 0


# Pose bar of the DEFAULT path against the direct path: 1e-5 in every rotation-matrix entry and 1e-5 m (10 um) in every translation component of every camera,
# marker and frame.  Measured at full size (profiles/r05_eta_pose_sweep.txt): cameras 3e-7 .. 5e-6, markers / frames 5e-7 .. 4e-6.  For scale: the direct path is
# 1.5e-4 / 6e-5 m away from the reference-faithful CPU run (analytic against central-difference float Jacobian), and the reference's own last LM step -- after
# which its stopping rule fires -- still moves the poses by 3e-3 / 1e-4 m.
POSE_BAR_CAMS, POSE_BAR_OTHERS = 1e-5, 1e-5
# ... and against the reference-faithful CPU run's final vector: the direct path's own distance from it (analytic against the reference's float-quantised
# central-difference Jacobian) is what the solver must not add to.  WHO carries that distance (profiles/r06_pose_delta_by_entity.txt, scripts/dev/
# pose_delta_by_entity.py): at config 3, full size, the cameras (1 560 .. 1 620 observations each) are within 2.6e-7 / 5.3e-7 m, the frames within 4.5e-6 / 1.5e-7,
# the markers within 1.6e-5 / 2.0e-6 -- the largest two markers are seen 84 and 96 times, the 20 markers seen 400 times and more stay below 1.0e-5.  On the
# 390-observation fixture g1_cfg2 the cameras (83 .. 112 observations) are at 1.5e-5 / 3.1e-5 and the worst entities are FRAMES with one marker in view
# (78 of 100 frames have 0 .. 4 observations: 4.4e-5).  The blanket bar below only remains for the two tau = 1e-6 fixtures, whose rejected tries depend on the last
# bits of a step (two direct runs part by as much); everything else gets the bars by entity kind.
POSE_BAR_FAITHFUL = 3e-4
POSE_BAR_FAITHFUL_FIXTURES = 2e-4                  # fixtures without rejected tries (measured: g1_cfg2 4.4e-5, g1_cfg3_cut 5.5e-5, the far start g1_cfg2_far 1.5e-4 -- frames with one marker in view)
POSE_BAR_FAITHFUL_CFG3 = {"cams": (2e-6, 2e-6), "markers": (5e-5, 1e-5), "frames": (2e-5, 2e-6)}   # config 3 at full size: (rotation-matrix entries, metres)


def _assert_poses_close(ds, x, x_direct, what, cams_bar=None):
    d = pose_delta(ds, x, x_direct)
    cr, ct = cams_bar if cams_bar is not None else (POSE_BAR_CAMS, POSE_BAR_CAMS)
    assert d["cams"][0] < cr and d["cams"][1] < ct, (what, d)
    assert max(d["markers"]) < POSE_BAR_OTHERS and max(d["frames"]) < POSE_BAR_OTHERS, (what, d)
    return d


@pytest.mark.parametrize("cfg", [3, 4, 5])
def test_default_options_reach_the_direct_paths_poses_at_full_size(cfg):
    # THE DEFAULT (aar_problem_create: NULL options -> AUTO -> SPCG at configs 3-4, PCG at config 5, default forcing terms) at BASELINE.json's
    # configurations, full size: same number of LM steps as the direct solver, final RMSE within 1e-6 px, final POSES as transforms within
    # 1e-6 (cameras) / 1e-5 (markers, frames) of the direct solver's
    ds = aar.synth(cfg)
    with aar.Problem(ds, solver="direct") as p:
        x_d, rep_d = p.lm_solve(ds.x_full)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds) as p:
        st0 = p.solver_stats()
        assert st0["solver"] == ("pcg" if cfg == 5 else "spcg") and st0["pcg_eta_loose"] == 0.0 and st0["env_overrides"] == 0
        x, rep = p.lm_solve(ds.x_full)
        rmse, _ = p.reproj_stats(x)
        st = p.solver_stats()
    assert rep["iterations"] == rep_d["iterations"], (rep["iterations"], rep_d["iterations"])
    assert abs(rmse - rmse_d) < 1e-6, (rmse, rmse_d)
    assert st["total_iterations"] > 0 and st["fallbacks"] <= 1
    # cameras: 1e-6 at configs 3 and 4 (measured 5e-8 / 3e-7 and 2e-7 / 4e-7); at config 5 the cameras' ROTATIONS are within 1e-6 too (3e-7), their translations
    # 4.7e-6 m (16 cameras around a 200-marker scene: the rig's scale is its weakest direction; forced SPCG ends 4.5e-6 away there as well): 1e-5 stated
    _assert_poses_close(ds, x, x_d, "config %d" % cfg, cams_bar=(1e-6, 1e-5 if cfg == 5 else 1e-6))


@pytest.mark.parametrize("name", ["g1_cfg2", "g1_cfg2_far", "g1_cfg2_retry", "g1_cfg2_huber", "g1_cfg2_huber_retry", "g1_cfg2_intr", "g1_cfg3_cut"])
def test_spcg_reaches_the_direct_paths_poses_on_every_fixture(name):
    # SPCG FORCED (AUTO keeps one-tile problems on the direct chain) at its default forcing term on every LM fixture -- far starts, tau = 1e-6 with
    # rejected tries, -with-huber (505 steps), the intrinsics block: final poses against the direct run and against the reference-faithful CPU run stored in
    # the fixture.  Same bar as at full size, except on the two tau = 1e-6 fixtures: there the damping starts at ~1e2, the first systems have a condition number
    # of ~1e9, the CG runs into its iteration cap and the direct chain takes those tries over (fall-backs), and WHICH try the gain test rejects depends on the
    # last bits of the step -- two direct runs with differently ordered atomic sums part ways by as much.  Their bar is the direct path's own distance from
    # the reference-faithful run on these fixtures (3e-4).
    ds, g = load_golden(name)
    huber, intr = "huber" in name, name.endswith("_intr")
    prm = aar.lm_default_params(tau=float(g["tau"][0])) if "tau" in g else None
    kw = dict(with_huber=huber, intrinsics=intr)
    with aar.Problem(ds, solver="direct", **kw) as p:
        x0 = p.x_with_intrinsics(ds.x_full) if intr else ds.x_full
        x_d, rep_d = p.lm_solve(x0, params=prm, trace_cap=600)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds, solver="spcg", **kw) as p:
        x, rep = p.lm_solve(x0, params=prm, trace_cap=600)
        rmse, _ = p.reproj_stats(x)
    assert abs(rmse - rmse_d) < 1e-6, (rmse, rmse_d)
    if not intr:       # (with the intrinsics block the direct path itself ends 2.8e-4 px from the faithful run: its central differences see the distortion columns)
        assert abs(rmse - g["faithful_rmse"][0]) < 1e-4, (rmse, g["faithful_rmse"][0])
    assert abs(rep["iterations"] - rep_d["iterations"]) <= (1 if "retry" in name else 0)
    d = pose_delta(ds, x, x_d)
    bar = POSE_BAR_FAITHFUL if "retry" in name else POSE_BAR_OTHERS
    assert max(d["cams"]) < bar and max(d["markers"]) < bar and max(d["frames"]) < bar, d
    if not huber and not intr:      # (the -with-huber fixtures' faithful run weights by another residual than the fp64 statistics: their poses are compared with the direct run only)
        f = pose_delta_max(ds, x, g["faithful_x"])
        f_d = pose_delta_max(ds, x_d, g["faithful_x"])
        assert max(f) < (POSE_BAR_FAITHFUL if "retry" in name else POSE_BAR_FAITHFUL_FIXTURES) and max(f) < max(f_d) + 3e-5, (f, f_d)


def test_auto_at_full_size_config3_against_compiled_reference_and_direct_path():
    # BASELINE.json's metric configuration through solver = AUTO (which is SPCG there): the bar of test_full_size_config3_against_compiled_reference
    # (final RMSE within 1e-4 px of the reference-faithful CPU run by the REAL SparseLevMarq), within 1e-5 px of the direct path, the same number of LM
    # steps, no try redone by the direct chain
    ds = aar.synth(3)
    o = ol.Oracle(ds)
    solve = o.ref_lm_solve if ol.have_ref() else o.lm_solve
    x_ref, rep_ref = solve(ds.x_full, jac_mode=ol.JAC_NUMERIC_F32, res_mode=ol.RES_F32, threads=min(32, os.cpu_count() or 1))
    with aar.Problem(ds, solver="direct") as p:
        x_d, rep_d = p.lm_solve(ds.x_full)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds) as p:      # the library's default options
        assert p.solver_stats()["solver"] == "spcg"
        x, rep = p.lm_solve(ds.x_full)
        rmse, _ = p.reproj_stats(x)
        st = p.solver_stats()
    ref = o.reproj_stats(x_ref)["rmse"]
    assert abs(rmse - ref) < 1e-4, (rmse, ref)
    assert abs(rmse - rmse_d) < 1e-6, (rmse, rmse_d)
    # poses against the REAL reference solver's run (central-difference float Jacobian): the default path is where the direct path is
    f, f_d = pose_delta_max(ds, x, x_ref), pose_delta_max(ds, x_d, x_ref)
    assert max(f) < POSE_BAR_FAITHFUL and max(f) < max(f_d) + 3e-5, (f, f_d)
    # ... by entity kind (the cameras carry almost none of it; the markers seen fewest carry the most)
    for xx in (x, x_d):
        by = pose_delta(ds, xx, x_ref)
        for kind, (br, bt) in POSE_BAR_FAITHFUL_CFG3.items():
            assert by[kind][0] < br and by[kind][1] < bt, (kind, by)
    assert rep["iterations"] == rep_d["iterations"] and abs(rep["iterations"] - rep_ref["iterations"]) <= 1
    assert all(t["tries"] == 1 and t["accepted"] == 1 for t in rep["trace"])
    assert st["fallbacks"] == 0 and 0 < st["total_iterations"] <= 64 * st["solves"]
    np.testing.assert_allclose(rep["final_err"], rep_ref["final_err"], rtol=1e-4)


@pytest.mark.parametrize("name,huber", [("g1_cfg2_retry", False), ("g1_cfg2_far", False), ("g1_cfg2_huber_retry", True), ("g1_cfg3_cut", False)])
def test_spcg_through_the_retry_far_start_and_huber_fixtures(name, huber):
    # the fixtures whose rejected tries are where an inexact step could change the branch of libs/sparselevmarq.h:406-419: far starts, tau = 1e-6,
    # -with-huber with a rejected try.  The inexact run still takes its rejected tries and ends within 1e-4 px of the reference-faithful run
    ds, g = load_golden(name)
    prm = aar.lm_default_params(tau=float(g["tau"][0])) if "tau" in g else None
    with aar.Problem(ds, with_huber=huber, solver="direct") as p:
        x_d, rep_d = p.lm_solve(ds.x_full, params=prm, trace_cap=600)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds, with_huber=huber, solver="spcg") as p:
        x, rep = p.lm_solve(ds.x_full, params=prm, trace_cap=600)
        rmse, _ = p.reproj_stats(x)
        st = p.solver_stats()
    assert abs(rmse - g["faithful_rmse"][0]) < 1e-4, (rmse, g["faithful_rmse"][0])
    assert abs(rmse - rmse_d) < 1e-6
    if "retry" in name:
        assert max(t["tries"] for t in rep["trace"]) > 1 and max(t["tries"] for t in rep_d["trace"]) > 1
    assert rep["trial_points"] == sum(t["tries"] for t in rep["trace"])
    # (from a far start with tau = 1e-6 the number of steps is not a stable quantity: the direct path itself is given +- 2 against the real solver there)
    assert abs(rep["iterations"] - rep_d["iterations"]) <= max(1 if "retry" in name else 0, rep_d["iterations"] // 100)
    assert 0 < st["solves"] <= rep["trial_points"] + st["fallbacks"]       # (after a fall-back the direct chain keeps the next tries)


def test_spcg_iteration_cap_falls_back_to_the_direct_chain():
    # a cap of one iteration at a forcing term nobody reaches in one: the first try of every solve raises device flag 8 and is redone by the direct chain,
    # which then keeps the rest of the LM run (the damping only falls along accepted steps: the systems get harder) -- the run is the direct run (to the
    # rounding of rebuilt blocks), and says how often it fell back
    ds, g = load_golden("g1_cfg3_cut")
    with aar.Problem(ds, solver="direct") as p:
        x_d, rep_d = p.lm_solve(ds.x_full)
        d_d = p.eval_damped_step(ds.x_full, 1e4)
    with aar.Problem(ds, solver="spcg", pcg_eta=1e-12, pcg_max_it=1) as p:
        x, rep = p.lm_solve(ds.x_full)
        st = p.solver_stats()
        # (try 1 only: a solve that came within 20 % of its cap announces that the next systems -- the damping only falls -- will not fit either; the rest of the LM run
        #  takes the direct chain without trying)
        assert st["fallbacks"] == 1 and st["solves"] == 1 and rep["trial_points"] == sum(t["tries"] for t in rep["trace"]) == 15
        x2, rep2 = p.lm_solve(ds.x_full)
        assert p.solver_stats()["fallbacks"] == 2 and p.solver_stats()["solves"] == 2          # every solve starts with its own solver again
        d = p.eval_damped_step(ds.x_full, 1e4)
        assert p.solver_stats()["fallbacks"] == 3
    assert rep["iterations"] == rep_d["iterations"]
    np.testing.assert_allclose([t["err"] for t in rep["trace"]], [t["err"] for t in rep_d["trace"]], rtol=1e-7)      # (the bar of the direct path's own traces: fp64 atomics)
    np.testing.assert_allclose(x, x_d, atol=1e-7)
    assert _rel(d, d_d) < 1e-11


def test_spcg_handover_timeout_falls_back_to_the_direct_chain():
    # a wavefront of the CG grid that never shows up (aar_problem_set_test_hook, AAR_TEST_HOOK_SPCG_DROP: what a device shared with another process can
    # do): the others give up after ~1 s, raise device flag 4, and the try is redone by the direct chain -- no error, no hang, the same step
    ds, g = load_golden("g1_cfg3_cut")
    with aar.Problem(ds, solver="direct") as p:
        d_d = p.eval_damped_step(ds.x_full, 1e6)
    with aar.Problem(ds, solver="spcg", pcg_eta=1e-9) as p:
        p.set_test_hook(aar.TEST_HOOK_SPCG_DROP, 5)
        d = p.eval_damped_step(ds.x_full, 1e6)
        assert p.solver_stats()["fallbacks"] == 1
        p.set_test_hook(aar.TEST_HOOK_SPCG_DROP, -1)
        d2 = p.eval_damped_step(ds.x_full, 1e6)                  # (the hook cleared: the same problem's next solve is a CG solve again, on clean hand-over buffers)
        assert p.solver_stats()["fallbacks"] == 1 and 0 < p.solver_stats()["last_iterations"] < 64
    assert _rel(d, d_d) < 1e-11 and _rel(d2, d_d) < 1e-6
    with pytest.raises(aar.AarError):
        with aar.Problem(ds, solver="spcg") as p:
            p.set_test_hook(99, 0)
    with aar.Problem(ds, solver="spcg", pcg_eta=1e-9) as p:       # (and the next problem's hand-over buffers are clean)
        d8 = p.eval_damped_step(ds.x_full, 1e8)
        assert p.solver_stats()["fallbacks"] == 0 and 0 < p.solver_stats()["last_iterations"] < 64
    with aar.Problem(ds, solver="direct") as p:
        assert _rel(d8, p.eval_damped_step(ds.x_full, 1e8)) < 1e-6


def test_problems_with_different_solvers_live_side_by_side_in_one_process():
    # the solver is a property of the problem (aar_solver_options), not of the process: three problems of one process, stepped in turn
    ds, g = load_golden("g1_cfg3_cut")
    alone = {}
    for s in ("direct", "spcg", "pcg"):
        with aar.Problem(ds, solver=s) as p:
            alone[s] = p.lm_solve(ds.x_full)
    ps = {s: aar.Problem(ds, solver=s) for s in ("direct", "spcg", "pcg")}
    try:
        assert [ps[s].solver_stats()["solver"] for s in ("direct", "spcg", "pcg")] == ["direct", "spcg", "pcg"]
        for s in ps:
            ps[s].lm_init(ds.x_full)
        errs = {s: [] for s in ps}
        for k in range(max(r["iterations"] for _, r in alone.values())):
            for s in ps:
                if k < alone[s][1]["iterations"]:
                    errs[s].append(ps[s].lm_step()["err"])
        for s in ps:
            np.testing.assert_allclose(errs[s], [t["err"] for t in alone[s][1]["trace"]], rtol=1e-6 if s == "direct" else 1e-4, err_msg=s)
        assert ps["direct"].solver_stats()["total_iterations"] == 0 and ps["spcg"].solver_stats()["total_iterations"] > 0 and ps["pcg"].solver_stats()["total_iterations"] > 0
    finally:
        for p in ps.values():
            p.close()


# Each part in a fresh process: the dynamic LDS a kernel may use is process-wide state, and any PCG solve before the side-by-side sequence (the solo runs,
# earlier tests) would already have raised it.  Problem 1 (A = 160) launches k_pcgf at 104 896 B; problem 2 (A = 200) is created, and its grid sizing opts
# the kernels in at ITS footprint; problem 1 then launches again before problem 2 does (problem 2's own launch, at 127 936 B, would raise the limit again).
_PCG_TWO_SIZES_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import aar
dss = [aar.synth(5, num_frames=300, num_markers=m) for m in (144, 184)]
if sys.argv[2] == "alone":
    out = []
    for ds in dss:
        with aar.Problem(ds, solver="pcg") as p:
            out.append([t["err"] for t in p.lm_solve(ds.x_full)[1]["trace"]])
else:
    steps = json.loads(sys.argv[2])
    ps = [aar.Problem(dss[0], solver="pcg")]
    ps[0].lm_init(dss[0].x_full)
    errs = [[ps[0].lm_step()["err"]], []]
    ps.append(aar.Problem(dss[1], solver="pcg"))
    ps[1].lm_init(dss[1].x_full)
    for _ in range(max(steps)):
        for i in (0, 1):
            if len(errs[i]) < steps[i]:
                errs[i].append(ps[i].lm_step()["err"])
    out = {"errs": errs, "solvers": [p.solver_stats()["solver"] for p in ps]}
    for p in ps:
        p.close()
print(json.dumps(out))
"""


def _pcg_two_sizes_child(mode):
    import json
    import subprocess
    import sys
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(aar.__file__)))
    out = subprocess.run([sys.executable, "-c", _PCG_TWO_SIZES_CHILD, pkg, mode], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith(("{", "["))][-1])


def test_pcg_problems_of_different_sizes_live_side_by_side_in_one_process():
    import json
    alone = _pcg_two_sizes_child("alone")
    assert len(alone[0]) >= 2 and len(alone[1]) >= 1, alone   # (problem 1 steps again after problem 2's creation)
    side = _pcg_two_sizes_child(json.dumps([len(t) for t in alone]))
    assert side["solvers"] == ["pcg", "pcg"]
    for i in (0, 1):
        np.testing.assert_allclose(side["errs"][i], alone[i], rtol=1e-4, err_msg=str(i))


@pytest.mark.parametrize("cfg", [3, 4, 5])
def test_inexact_solvers_at_full_size_against_the_direct_path(cfg):
    # configs 3, 4, 5 at FULL size: PCG through the frame blocks (what AUTO picks at config 5) and, where the reduced system fits the wavefronts'
    # registers, CG on the explicit system (what AUTO picks at configs 3 and 4): final RMSE within 1e-5 px of the direct path, LM steps <= direct + 1
    ds = aar.synth(cfg)
    with aar.Problem(ds, solver="direct") as p:
        x_d, rep_d = p.lm_solve(ds.x_full)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds, solver="auto") as p:
        auto = p.solver_stats()["solver"]
    assert auto == ("pcg" if cfg == 5 else "spcg")
    for s in ("pcg", "spcg"):
        with aar.Problem(ds, solver=s) as p:
            x, rep = p.lm_solve(ds.x_full)
            rmse, _ = p.reproj_stats(x)
            st = p.solver_stats()
        assert abs(rmse - rmse_d) < 1e-6, (cfg, s, rmse, rmse_d)
        assert rep["iterations"] == rep_d["iterations"], (cfg, s)
        d = pose_delta(ds, x, x_d)
        assert max(max(v) for v in d.values()) < 3e-5, (cfg, s, d)      # (also the solver AUTO does not pick at this size)
        assert st["total_iterations"] > 0 and (s == "pcg" or st["fallbacks"] <= 1)


def _run_ranks(world, fn):
    grp = aar.LocalGroup(world)
    out, errs = [None] * world, []
    def run(rank):
        try:
            comm = aar.Comm.local(grp, rank)
            try:
                out[rank] = fn(comm, rank)
            finally:
                comm.close()
        except Exception as e:      # noqa: BLE001
            errs.append((rank, e))
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    grp.close()
    assert not errs, errs
    return out


def test_config5_shaped_problem_against_the_oracle():
    # config 5's entity count (16 cameras / 200 markers: 14 tiles of LDL^T, MFMA Schur kernel, look-ahead, pass A in 128-thread workgroups) on a cut of
    # 300 frames the oracle can factor (75 612 marker observations): residual rows bit for bit, the damped step at two dampings against the oracle's sparse
    # LDL^T, the LM run against the oracle's (analytic Jacobian) -- direct, PCG and CG on the explicit system, on one rank and on four
    ds = aar.synth(5, num_frames=300)
    o = ol.Oracle(ds)
    do = {mu: o.damped_solve(ds.x_full, mu, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32) for mu in (1e3, 1e7)}
    xo, repo = o.lm_solve(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F32)
    rmse_o = o.reproj_stats(xo)["rmse"]
    with aar.Problem(ds, solver="direct") as p:
        r, ss = p.eval_residuals(ds.x_full)
        assert np.array_equal(r, o.residuals(ds.x_full, res_mode=ol.RES_F32))
        for mu, d_ref in do.items():
            assert _rel(p.eval_damped_step(ds.x_full, mu), d_ref) < 1e-8, mu
        x, rep = p.lm_solve(ds.x_full)
        rmse, _ = p.reproj_stats(x)
    assert rep["iterations"] == repo["iterations"]
    np.testing.assert_allclose([t["err"] for t in rep["trace"]], [t["err"] for t in repo["trace"]], rtol=1e-6)
    assert abs(rmse - rmse_o) < 1e-7
    for s, eta in (("pcg", 1e-11), ("spcg", 1e-12)):
        with aar.Problem(ds, solver=s, pcg_eta=eta, pcg_max_it=2000) as p:
            for mu, d_ref in do.items():
                assert _rel(p.eval_damped_step(ds.x_full, mu), d_ref) < 1e-7, (s, mu)
    for s in ("pcg", "spcg"):
        with aar.Problem(ds, solver=s) as p:
            x, rep = p.lm_solve(ds.x_full)
            assert abs(p.reproj_stats(x)[0] - rmse_o) < 1e-6, s        # (north star: 1e-4)
            assert abs(rep["iterations"] - repo["iterations"]) <= 1, s
            assert max(pose_delta_max(ds, x, xo)) < 3e-5, s            # final poses against the ORACLE's run (analytic Jacobian, sparse LDL^T)
    for s in ("direct", "pcg", "spcg"):
        def solve(comm, rank, s=s):
            with aar.Problem(ds, comm=comm, solver=s) as q:
                xs, reps = q.lm_solve(ds.x_full)
                return q.reproj_stats(xs)[0], reps
        for rmse_r, reps in _run_ranks(4, solve):
            assert abs(rmse_r - rmse_o) < (1e-7 if s == "direct" else 1e-6), (s, rmse_r, rmse_o)
            assert abs(reps["iterations"] - repo["iterations"]) <= 1, s


def test_init_head_start_leaves_the_trajectory_alone(monkeypatch):
    # aar_lm_init queues the first step's frame inverses and Schur complement before the host has read mu_0 (AAR_INIT_HEADSTART, a per-problem
    # tuning switch): with fixed-order sums the whole LM run is the same bit for bit with and without it -- also when the step then wants another
    # damping than the one the head start assumed (tau changed between init and step: the complement is taken back and redone)
    ds, g = load_golden("g1_cfg3_cut")
    runs = {}
    for hs in ("1", "0"):
        monkeypatch.setenv("AAR_INIT_HEADSTART", hs)
        with aar.Problem(ds, deterministic=True, solver="direct") as p:
            x, rep = p.lm_solve(ds.x_full)
            p.lm_init(ds.x_full, params=aar.lm_default_params(tau=1.0))
            p.lm_init(ds.x_full, params=aar.lm_default_params(tau=1e-3))     # a second init: the first one's head start is discarded
            steps = [p.lm_step() for _ in range(4)]
            runs[hs] = (x, [t["err"] for t in rep["trace"]], [t["mu"] for t in rep["trace"]], [s["err"] for s in steps], [s["mu"] for s in steps])
    monkeypatch.delenv("AAR_INIT_HEADSTART")
    for a, b in zip(runs["1"], runs["0"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    np.testing.assert_allclose(runs["1"][1], g["analytic_err"], rtol=1e-7)


def test_cpp_mirror_and_driver_take_the_solver_as_an_option(tmp_path):
    # aar::MultiCamMapper::set_solver_options (beside SparseLevMarq::Params, libs/sparselevmarq.h:30-50) through the driver.  WITHOUT a flag aar_find_solution
    # runs the library's default (AUTO): the direct chain on a 4-camera / 12-marker recording (one tile of unknowns), SPCG on BASELINE.json's metric
    # configuration (8 cameras / 40 markers / 500 frames) -- where its final.solution holds the poses `-solver direct` ends at
    import subprocess
    from conftest import PKG
    exe = os.path.join(PKG, "aar_find_solution")
    runs = {}
    for s in ("default", "direct", "spcg"):
        folder = str(tmp_path / s)
        assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
        run = subprocess.run([exe, folder, "0.05", "x", "-from-initial"] + ([] if s == "default" else ["-solver", s]), capture_output=True, text=True)
        assert run.returncode == 0, run.stderr + run.stdout
        fin = aar.solution_read(os.path.join(folder, "final.solution"))
        runs[s] = (ol.Oracle(fin).reproj_stats(fin.x_full)["rmse"], run.stdout, fin)
    assert "solver: spcg" in runs["spcg"][1] and "CG iterations" in runs["spcg"][1] and "solver: direct" in runs["direct"][1]
    assert "solver: direct" in runs["default"][1]                      # (one tile of unknowns: AUTO keeps the direct chain)
    assert abs(runs["spcg"][0] - runs["direct"][0]) < 1e-6 and abs(runs["default"][0] - runs["direct"][0]) < 1e-9
    assert max(pose_delta_max(runs["direct"][2], runs["spcg"][2].x_full, runs["direct"][2].x_full)) < POSE_BAR_OTHERS
    bad = subprocess.run([exe, str(tmp_path / "direct"), "0.05", "x", "-solver", "nonsense"], capture_output=True, text=True)
    assert bad.returncode != 0
    big = {}
    for s in ("default", "direct"):
        folder = str(tmp_path / ("cfg3_" + s))
        assert subprocess.run([exe, "--synth", "3", folder], capture_output=True, text=True).returncode == 0
        run = subprocess.run([exe, folder, "0.05", "x", "-from-initial"] + ([] if s == "default" else ["-solver", s]), capture_output=True, text=True)
        assert run.returncode == 0, run.stderr + run.stdout
        big[s] = (run.stdout, aar.solution_read(os.path.join(folder, "final.solution")))
    assert "solver: spcg" in big["default"][0] and "solver: direct" in big["direct"][0]
    _assert_poses_close(big["direct"][1], big["default"][1].x_full, big["direct"][1].x_full, "aar_find_solution, config 3")


def test_spcg_in_deterministic_mode_gives_the_same_bits_twice():
    # k_spcg has no atomics (every wavefront adds the same shares in the same order); with fixed-order sums in the passes and the Schur kernel the whole
    # INEXACT run -- CG iteration counts included -- is bit-reproducible, on one rank and on two
    ds, g = load_golden("g1_cfg3_cut")
    def run():
        with aar.Problem(ds, solver="spcg", deterministic=True) as p:
            x, rep = p.lm_solve(ds.x_full)
            return x, [t["err"] for t in rep["trace"]], [t["mu"] for t in rep["trace"]], p.solver_stats()["total_iterations"]
    a, b = run(), run()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[3] == b[3] > 0
    def solve(comm, rank):
        with aar.Problem(ds, comm=comm, solver="spcg", deterministic=True) as q:
            xs, reps = q.lm_solve(ds.x_full)
            return xs, [t["err"] for t in reps["trace"]]
    r1, r2 = _run_ranks(2, solve), _run_ranks(2, solve)
    for (xa, ea), (xb, eb) in zip(r1, r2):
        assert np.array_equal(xa, xb) and ea == eb
    assert np.array_equal(r1[0][0], r1[1][0])
    np.testing.assert_allclose(r1[0][1], a[1], rtol=1e-5)     # (one rank against two: another order of the sums, a CG solve stopped an iteration apart)


def test_solver_options_struct_is_forward_compatible_and_validated():
    # aar_solver_options carries its own size: a caller built against a shorter struct (only struct_size + solver) keeps working, the fields it does not know
    # take their defaults; an unset struct_size and values outside the enums are refused with AAR_ERR_INVALID (no silent fall-back to another solver)
    import ctypes as C
    ds, g = load_golden("g1_cfg3_cut")
    cds = ds.as_c()
    d = aar.CProblemDesc()
    aar.lib().aar_problem_desc_from_dataset(C.byref(cds), C.byref(d))
    so = aar.CSolverOptions()
    aar.lib().aar_solver_default_options(C.byref(so))
    assert so.struct_size == C.sizeof(aar.CSolverOptions) and so.solver == aar.SOLVER_AUTO and so.deterministic == 0 and so.pcg_eta == 0.0 and so.pcg_eta_loose == 0.0 and so.pcg_abs_tol == 0.0
    h = C.c_void_p()
    so.solver, so.struct_size, so.deterministic, so.pcg_eta = aar.SOLVER_SPCG, 8, 1, 0.5      # a "short" caller: deterministic / eta lie beyond its struct
    assert aar.lib().aar_problem_create_ex(C.byref(d), C.byref(so), C.byref(h)) == 0
    st = aar.CSolverStats()
    assert aar.lib().aar_problem_get_solver_stats(h, C.byref(st)) == aar.AAR_ERR_INVALID      # the caller must say how large ITS struct is
    st.struct_size = C.sizeof(aar.CSolverStats)
    assert aar.lib().aar_problem_get_solver_stats(h, C.byref(st)) == 0
    assert st.solver == aar.SOLVER_SPCG and st.deterministic == 0 and abs(st.pcg_eta - 3e-4) < 1e-18 and st.pcg_eta_loose == 0.0 and st.env_overrides == 0 and st.pcg_abs_tol == 2e-5
    # a caller built against a SHORTER stats struct: nothing beyond its size is written
    buf = (C.c_uint8 * C.sizeof(aar.CSolverStats))(*([0xAB] * C.sizeof(aar.CSolverStats)))
    short = C.cast(buf, C.POINTER(aar.CSolverStats))
    short.contents.struct_size = 48
    assert aar.lib().aar_problem_get_solver_stats(h, short) == 0
    assert short.contents.solver == aar.SOLVER_SPCG and all(b == 0xAB for b in bytes(buf)[48:])
    aar.lib().aar_problem_destroy(h)
    for bad in (dict(struct_size=0), dict(solver=7), dict(pcg_eta=-1.0), dict(pcg_max_it=-3), dict(pcg_eta_loose=-0.5), dict(pcg_eta_switch=-1.0), dict(pcg_abs_tol=-1e-6)):
        aar.lib().aar_solver_default_options(C.byref(so))
        for k, v in bad.items():
            setattr(so, k, v)
        h = C.c_void_p()
        assert aar.lib().aar_problem_create_ex(C.byref(d), C.byref(so), C.byref(h)) == aar.AAR_ERR_INVALID, bad
    # a solver the problem is too large for is refused, not replaced: CG on the explicit system beyond 14 tiles of unknowns
    big = aar.synth(3, num_cams=4, num_markers=300, num_frames=12)
    with pytest.raises(aar.AarError) as e:
        aar.Problem(big, solver="spcg")
    assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    with aar.Problem(big, solver="auto") as p:
        assert p.solver_stats()["solver"] == "pcg"


def test_environment_overrides_only_fill_defaults_and_are_reported(monkeypatch):
    # AAR_SOLVER / AAR_PCG_ETA are bisecting aids: they apply where the caller left the field at its default and never override an explicit choice;
    # aar_solver_stats.env_overrides says what they changed
    ds, g = load_golden("g1_cfg3_cut")
    monkeypatch.setenv("AAR_SOLVER", "pcg")
    monkeypatch.setenv("AAR_PCG_ETA", "0.05")
    with aar.Problem(ds) as p:
        st = p.solver_stats()
        assert st["solver"] == "pcg" and st["pcg_eta"] == 0.05 and st["env_overrides"] == aar.ENV_SOLVER | aar.ENV_PCG_ETA
    with aar.Problem(ds, solver="direct") as p:
        st = p.solver_stats()
        assert st["solver"] == "direct" and not (st["env_overrides"] & aar.ENV_SOLVER)
    with aar.Problem(ds, solver="spcg", pcg_eta=1e-3) as p:
        st = p.solver_stats()
        assert st["solver"] == "spcg" and st["pcg_eta"] == 1e-3 and st["env_overrides"] == 0


def test_forcing_sequence_is_an_option():
    # pcg_eta_loose > pcg_eta: the early LM steps (while the last accepted step took more than pcg_eta_switch of the error away) are solved to pcg_eta_loose,
    # the late ones to pcg_eta -- fewer CG iterations, the same number of LM steps, the final error within 1e-5 px of the direct solver's; the poses of such
    # a run are measurably further from the direct run's (which is why it is not the default: kernels.h, profiles/r05_eta_pose_sweep.txt)
    ds = aar.synth(3)
    with aar.Problem(ds, solver="direct") as p:
        xd, rd = p.lm_solve(ds.x_full)
        rmse_d = p.reproj_stats(xd)[0]
    out = {}
    loose = dict(pcg_eta_loose=0.1, pcg_eta=0.02, pcg_abs_tol=1.0)      # (round 4's defaults; the absolute tolerance out of the way as well)
    for name, kw in (("default", {}), ("sequence", loose), ("sequence_never", dict(loose, pcg_eta_switch=1e9))):
        with aar.Problem(ds, **kw) as p:
            st = p.solver_stats()
            assert st["solver"] == "spcg" and st["pcg_eta_loose"] == (0.0 if name == "default" else 0.1)
            x, rep = p.lm_solve(ds.x_full)
            st = p.solver_stats()
            out[name] = (p.reproj_stats(x)[0], rep["iterations"], st["total_iterations"], st["fallbacks"], max(pose_delta_max(ds, x, xd)))
    for name, (rmse, its, cg, fb, dp) in out.items():
        assert abs(rmse - rmse_d) < 1e-5 and its == rd["iterations"] and fb == 0, (name, rmse, rmse_d, its)
    assert out["sequence"][2] < out["sequence_never"][2] < out["default"][2]
    assert out["default"][4] < POSE_BAR_OTHERS < out["sequence"][4]


@pytest.mark.parametrize("scale,tau", [(3.0, 1.0), (1.0, 1e-6), (3.0, 1e-6)])
def test_default_options_from_far_starts_and_tiny_initial_damping(scale, tau):
    # The relative forcing term alone lets an inner solve stop while the step is still LARGE in absolute terms -- a start 3x further out, or tau = 1e-6 (a tiny initial
    # damping: three Gauss-Newton-like steps through systems of condition ~1e9): what it leaves out lands in the final poses (measured without the absolute tolerance:
    # 2e-5 at x3, 4e-3 .. 1e-2 at tau = 1e-6).  aar_solver_options.pcg_abs_tol (default 2e-5 / 5e-5, in pose units) is the second condition an inner solve has to meet:
    # the CG runs on, or hands the try to the direct chain at its iteration cap.  Full-size config 3: same LM steps, RMSE within 1e-6 px, poses within 3e-5.
    ds = aar.synth(3, init_scale=scale)
    prm = aar.lm_default_params(tau=tau)
    with aar.Problem(ds, solver="direct") as p:
        x_d, rep_d = p.lm_solve(ds.x_full, params=prm)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds) as p:
        assert p.solver_stats()["solver"] == "spcg" and p.solver_stats()["pcg_abs_tol"] == 2e-5
        x, rep = p.lm_solve(ds.x_full, params=prm)
        rmse, _ = p.reproj_stats(x)
    assert rep["iterations"] == rep_d["iterations"] and abs(rmse - rmse_d) < 1e-6, (rep["iterations"], rep_d["iterations"], rmse, rmse_d)
    assert max(pose_delta_max(ds, x, x_d)) < 3e-5, pose_delta_max(ds, x, x_d)
    if tau < 1.0:      # ... and what the absolute tolerance is there for
        with aar.Problem(ds, pcg_abs_tol=1.0) as p:
            x_rel, _ = p.lm_solve(ds.x_full, params=prm)
        assert max(pose_delta_max(ds, x_rel, x_d)) > 1e-4


def test_auto_resolves_to_the_same_solver_on_every_rank_of_a_lopsided_sharding():
    # AUTO's choice between SPCG and PCG rests on (entity, frame) incidences.  Decided from a rank's OWN frames, the ranks of this data set would split --
    # rank 0 owns frames that see ~120 entities each (incidences x (per frame - 30) >= 4e6: PCG), rank 1 mostly frames that see a dozen (SPCG) -- and wait in
    # different collectives forever.  The rule is applied to the whole data set's numbers, the same on every rank: asserted right after creation, then solved
    dense = 3000
    ds = aar.synth(5, num_frames=7000)
    keep = ~((ds.obs_frame >= dense) & ((ds.obs_marker >= 12) | (ds.obs_cam >= 4)))
    for name in ("obs_frame", "obs_cam", "obs_marker", "obs_uv"):
        setattr(ds, name, getattr(ds, name)[keep])
    ds.num_obs = int(keep.sum())
    begin = aar.plan_shards(np.bincount(ds.obs_frame, minlength=ds.num_frames), 2)
    inc_c = np.unique(ds.obs_frame.astype(np.int64) * 4096 + ds.obs_cam) // 4096
    inc_m = np.unique(ds.obs_frame.astype(np.int64) * 4096 + ds.obs_marker) // 4096
    def own_rule(lo, hi):      # the rule of csrc/ba_capi.hip on the frames lo .. hi alone
        slots = int(((inc_c >= lo) & (inc_c < hi)).sum() + ((inc_m >= lo) & (inc_m < hi)).sum())
        return slots * (slots / (hi - lo) - 30.0) >= 4e6
    assert own_rule(begin[0], begin[1]) and not own_rule(begin[1], begin[2])        # (decided per rank, the two would part)

    def create(comm, rank):
        with aar.Problem(ds, comm=comm) as q:
            return q.solver_stats()["solver"]
    out = _run_ranks(2, create)
    assert out[0] == out[1] and out[0] in ("spcg", "pcg"), out
    prm = lambda: aar.lm_default_params(max_iters=3)
    with aar.Problem(ds, solver=out[0]) as p:
        x, rep = p.lm_solve(ds.x_full, params=prm())
    def solve(comm, rank):
        with aar.Problem(ds, comm=comm) as q:
            xs, reps = q.lm_solve(ds.x_full, params=prm())
            return [t["err"] for t in reps["trace"]]
    res = _run_ranks(2, solve)
    assert res[0] == res[1]                                          # same trace on both ranks, bit for bit
    np.testing.assert_allclose(res[0], [t["err"] for t in rep["trace"]], rtol=1e-6)


def test_pcg_with_fp32_blocks_ends_where_the_fp64_blocks_do(monkeypatch):
    # PCG at the default forcing term reads W in fp32 (pass A writes a piece-major fp32 copy instead of the fp64 blocks; k_pcgf's set-up, its operator and the
    # back-substitution read it): the final poses are those of the fp64 blocks (AAR_PCG_W32=0) to far below the bar, a forcing term below 1e-4 gets fp64 blocks by
    # itself, and the dense-output API still sees fp64 W (config 5's shape on a 300-frame cut; full size: test_default_options_reach_the_direct_paths_poses...)
    ds = aar.synth(5, num_frames=300)
    with aar.Problem(ds, solver="direct") as p:
        xd, repd = p.lm_solve(ds.x_full)
        Hd, Bd, _ = p.eval_normal_equations(ds.x_full)
    with aar.Problem(ds, solver="pcg") as p:
        x32, rep32 = p.lm_solve(ds.x_full)
        rm32, _ = p.reproj_stats(x32)
        H, B, _ = p.eval_normal_equations(ds.x_full)               # (asks pass A for the fp64 blocks again)
        assert np.abs(H - Hd).max() / np.abs(Hd).max() < 1e-12 and np.abs(B - Bd).max() / np.abs(Bd).max() < 1e-12
        x32b, rep32b = p.lm_solve(ds.x_full)                        # ... and the solver is back on the fp32 copy afterwards
        assert rep32b["iterations"] == rep32["iterations"] and max(pose_delta_max(ds, x32b, x32)) < 1e-6
    monkeypatch.setenv("AAR_PCG_W32", "0")
    with aar.Problem(ds, solver="pcg") as p:
        x64, rep64 = p.lm_solve(ds.x_full)
        rm64, _ = p.reproj_stats(x64)
    monkeypatch.delenv("AAR_PCG_W32")
    assert rep32["iterations"] == rep64["iterations"] == repd["iterations"]
    assert abs(rm32 - rm64) < 1e-7
    assert max(pose_delta_max(ds, x32, x64)) < 2e-6, pose_delta_max(ds, x32, x64)
    assert max(pose_delta_max(ds, x32, xd)) < 3e-5
    with aar.Problem(ds, solver="pcg", pcg_eta=1e-9, pcg_max_it=2000) as p:        # tight forcing term: fp64 blocks, the direct step to 1e-7
        mu = 1e5
        with aar.Problem(ds, solver="direct") as q:
            d_ref = q.eval_damped_step(ds.x_full, mu)
        assert _rel(p.eval_damped_step(ds.x_full, mu), d_ref) < 1e-7


def test_pcg_keeping_the_coarse_operator_between_solves_ends_where_forming_it_every_solve_does(monkeypatch):
    # k_pcgf forms Z^T S Z of its coarse space every third solve of an LM run and keeps it in between (AAR_PCG_E_EVERY; the damping's mu Z^T Z is always today's):
    # a preconditioner only has to be symmetric positive definite and fixed during a solve, so the solves end at the same forcing term -- the poses of the run
    # agree with forming it every solve far below the bar, at a few more CG iterations (config 5's shape on a 300-frame cut; the coarse space joins from
    # 8 iterations of the previous solve on, so the first LM steps never use it)
    ds = aar.synth(5, num_frames=300)
    out = {}
    for every in ("1", "3", "6"):
        monkeypatch.setenv("AAR_PCG_E_EVERY", every)
        with aar.Problem(ds, solver="pcg") as p:
            x, rep = p.lm_solve(ds.x_full)
            out[every] = (x, rep, p.solver_stats())
    monkeypatch.delenv("AAR_PCG_E_EVERY")
    x1, rep1, st1 = out["1"]
    assert st1["total_iterations"] > 4 * rep1["iterations"]         # (the problem is one where the coarse space is at work at all)
    for every in ("3", "6"):
        x, rep, st = out[every]
        assert rep["iterations"] == rep1["iterations"]
        assert max(pose_delta_max(ds, x, x1)) < 1e-5, (every, pose_delta_max(ds, x, x1))
        assert st["total_iterations"] < 1.5 * st1["total_iterations"], (every, st["total_iterations"], st1["total_iterations"])


@pytest.mark.parametrize("name", ["g1_cfg2", "g1_cfg2_far", "g1_cfg2_retry", "g1_cfg2_huber", "g1_cfg2_huber_retry", "g1_cfg2_intr", "g1_cfg3_cut"])
def test_pcg_with_its_fp32_blocks_reaches_the_direct_paths_poses_on_every_fixture(name):
    # PCG FORCED (AUTO never picks it at these sizes) at its default forcing term -- fp32 W blocks, k_pcgf -- on every LM fixture.  Its default term (5e-3 on |r| / |b|)
    # was chosen at config 5 (3.6e-6 there); on these 60- and 100-frame problems it ends 1.2e-5 .. 1.4e-5 from the direct run -- with fp64 blocks exactly as with fp32
    # ones (scripts/dev/pcg_w32_fixtures.py) -- so the bar is the 3e-5 of the other forced-solver test, not AUTO's 1e-5.  The intrinsics fixture (focal length against
    # depth: the weakest directions of all; 24 LM steps) ends 1e-3 away under PCG at this size, fp64 blocks or fp32: RMSE is asserted there, the poses get a stated 2e-3.
    # On the tau = 1e-6 fixtures which try the gain test rejects depends on the last bits of the step, as for SPCG.
    ds, g = load_golden(name)
    huber, intr = "huber" in name, name.endswith("_intr")
    prm = aar.lm_default_params(tau=float(g["tau"][0])) if "tau" in g else None
    kw = dict(with_huber=huber, intrinsics=intr)
    with aar.Problem(ds, solver="direct", **kw) as p:
        x0 = p.x_with_intrinsics(ds.x_full) if intr else ds.x_full
        x_d, rep_d = p.lm_solve(x0, params=prm, trace_cap=600)
        rmse_d, _ = p.reproj_stats(x_d)
    with aar.Problem(ds, solver="pcg", **kw) as p:
        x, rep = p.lm_solve(x0, params=prm, trace_cap=600)
        rmse, _ = p.reproj_stats(x)
        assert p.solver_stats()["pcg_eta"] == 5e-3
    assert abs(rmse - rmse_d) < (1e-5 if intr else 1e-6), (rmse, rmse_d)      # (north star: 1e-4 px; the intrinsics run ends 4e-6 px BELOW the direct run's error)
    assert abs(rep["iterations"] - rep_d["iterations"]) <= (2 if "retry" in name else 0), (rep["iterations"], rep_d["iterations"])
    d = pose_delta(ds, x, x_d)
    bar = 2e-3 if intr else (POSE_BAR_FAITHFUL if "retry" in name else 3e-5)
    assert max(d["cams"]) < bar and max(d["markers"]) < bar and max(d["frames"]) < bar, d
