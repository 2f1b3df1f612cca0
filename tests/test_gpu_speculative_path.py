"""The speculative step path of the LM loop, certified in every launch shape -- damped_try (csrc/ba_capi.hip) predicts that an accepted step is
followed by one at 0.33 mu and makes that step's system ahead of time: pass A at the trial point inverts V_f + 0.33 mu I itself (passA_epilogue
and its wrench twin, csrc/eval_kernels.hip: Vinv, h_f, with the MFMA Schur kernel the panels Wd / Yd), the trial's Schur complement is subtracted
before the host has decided, behind a communicator S | rhs | g0 travels with the step's scalars, with AAR_SPEC_CHOL the factorisation is queued
too.  A correctly predicted try then runs none of k_frame_inv, k_schur_fill, k_schur.  Needs a real MI355X.

Every test is an LM run (solver="direct", at most ten steps) whose own steps are certified by tests/direct_run_certificate.py: z after every step
from the step callback, the device's own H, B evaluated AFTER the run at the recorded points, certify_direct (tests/direct_certificate.py: the bars
are that module's, nothing is added) on zs[k + 1] - zs[k] at the damping the trace implies.  The first six predicted steps are certified, none
skipped; every test states how many it must have certified (three) and fails when the run did not offer them -- which
tests/test_direct_run_certificate_host.py has found on the CPU for every run of direct_cases.SPEC_RUNS, so this module does not discover it here.
The tuning switches are read when the problem is created: monkeypatch.setenv before Problem(...) selects the launch shape.

Launch counts (one GPU, kernel profiling on: it keeps the first step's head start out of aar_lm_init and changes nothing else on one GPU):
k_frame_inv launches over the run == the tries that are not predicted, the run's first try among them.  k_schur_fill and the Schur kernels share
one counter, "k_schur", which counts launch_schur CALLS (one event pair around fill + MFMA kernel, or k_schur<0, 1> + k_schur_reduce): it must be
one per predicted try (the next trial's complement), two per other try, one more where a complement is taken back.  It tells that no complement
was formed for a predicted try; it does NOT tell whether an MFMA launch filled its panels or took pass A's (AAR_DENSE_FROM_PASSA) -- that is read
off panels_ok / eval_blocks, and the certificate is what checks the panels.  Ranks run without the profiler (it switches AAR_SPEC_CHOL off).

Ratios: every certified step's |r| / bar and worst frame ratio per family, printed when the module finishes (run with -s).
MEASURED on an MI355X (family: certified steps, worst, median |r| / bar; worst frame ratio):
    pass A instances     204   4.98e-2   8.7e-3    9.3e-3
    wide frames           24   1.36e-2   2.1e-3    1.7e-3
    dense panels         204   3.59e-2   2.1e-3    3.8e-3
    features              66   1.69e-1   1.1e-2    7.4e-3      (the worst is the intrinsics run; without it 3.3e-2, median 5.3e-3)
    deterministic         36   4.98e-2   5.3e-3    2.3e-3
    ranks                102   2.48e-2   7.2e-3    3.9e-3      (every rank of a run recorded the same bits: one certificate per run)
    ranks, small gain     18   1.9e-7    8.0e-9    2.1e-2
    repairs                9   1.1e-7    7.5e-9    6.0e-3
These are the ratios of plain float64 on the same runs, read back through z in the same way (tests/test_direct_run_certificate_host.py: 5.0e-2
on the pass A sets, 1.44e-1 with intrinsics, 7e-8 from the far start): what is left is the rounding of z1 = z0 + d, which the certificate's
slack allows for, and at tau = 1e-6 a bar of (a) that kappa_f ~ 1e6 makes wide -- there the frame part (c) is the part that bites.
Every predicted step passed, and k_frame_inv / launch_schur counts were what the classification implies in every single-GPU test.
Wall time: 106 tests in 5.8 s, the slowest 0.25 s.
"""
import ctypes as C

import numpy as np
import pytest

import aar
import direct_cases as dc
import direct_run_certificate as drc
from reduced_system import held_mask, slot_col

pytestmark = pytest.mark.gpu

NEED = 3                   # predicted steps every run must have certified
RATIOS = {}                # family -> [(|r| / bar, frame ratio)]
SWITCHES = ("AAR_PASSA_VARIANT", "AAR_PASSA_WRENCH", "AAR_MERGE_PASSES", "AAR_PASSAB_OCC2", "AAR_SCHUR_MFMA",
            "AAR_DENSE_FROM_PASSA", "AAR_SCHUR_SPLIT", "AAR_FUSED_COMM", "AAR_SPEC_CHOL")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_report():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")
    yield
    print("\nspeculative-path certificate ratios (family: steps, worst, median |r| / bar; worst frame ratio)")
    for fam, v in sorted(RATIOS.items()):
        a = np.array(v)
        print("  %-22s %4d  %.3e  %.3e   %.3e" % (fam, len(a), a[:, 0].max(), np.median(a[:, 0]), a[:, 1].max()))


def _env(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _merge_z(p, x0, z):
    """the full vector of the pose vector z (aar_problem_merge_z: what z does not hold stays as in x0)"""
    x = np.array(x0, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    assert z.shape == (p.num_vars,) and x.shape == (p.full_len,)
    assert aar.lib().aar_problem_merge_z(p.handle, z.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return x


class Run:
    """a named run of direct_cases.SPEC_RUNS: what a Problem of it needs, and how its recorded steps are certified"""

    def __init__(self, name):
        self.name = name
        self.ds, self.x0, self.kw, self.tau, need, self.huber = dc.spec_run(name)
        assert need == NEED
        self.opt, self.intr = self.kw.get("optimize", (True, True, True)), self.kw.get("intrinsics", False)
        self.fixed = {k: self.kw[k] for k in ("fixed_cams", "fixed_markers") if k in self.kw}
        self.params = aar.lm_default_params(tau=self.tau, max_iters=10)

    def problem(self, **over):
        p = aar.Problem(self.ds, solver="direct", **dict(self.kw, **over))
        assert p.solver_stats()["solver"] == "direct"
        if self.huber is not None:
            p.set_huber_delta(self.huber)     # (a fixed delta: with a caller's step callback aar_lm_solve runs no schedule of its own)
        return p

    def mu0(self, p):
        """tau max diag H of the device's own H at the start (fixed entities' rows left out, as k_maxdiag leaves them out)"""
        H0, _, _ = p.eval_normal_equations(self.x0)
        held = held_mask(self.ds, len(H0), **self.fixed) if self.fixed else np.zeros(len(H0), bool)
        return self.tau * float(np.diag(H0)[~held].max())

    def certify(self, family, p, zs, trace, mu0, kinds=("predicted",), what=""):
        """certify the first six predicted steps (and three of every other kind asked for) against p's own H, evaluated now -- AFTER the run"""
        assert len(trace) <= 10 and len(zs) == len(trace) + 1
        ks, cls = drc.pick_steps(trace, kinds)
        drc.check_predicted_dampings(trace, mu0)
        res = drc.certify_steps(self.ds, zs, trace, mu0, p.eval_normal_equations, lambda z: _merge_z(p, self.x0, z), ks,
                                what="%s %s %s" % (family, self.name, what), optimize=self.opt, intrinsics=self.intr, fixed=self.fixed)
        assert sum(c == "predicted" for _, c, _ in res) >= NEED, (self.name, what, cls)      # the premise
        for _, _, out in res:
            RATIOS.setdefault(family, []).append((out["ratio"], out["frame_ratio"]))
        return res, cls

    def run_one_gpu(self, family, kinds=("predicted",), what="", **over):
        """the run on one GPU under the kernel profiler; asserts the launch counts its trace implies, then certifies.  Returns (zs, trace, classes)"""
        with self.problem(**over) as p:
            assert p.solver_stats()["deterministic"] == bool(over.get("deterministic", False))
            p.set_kernel_profiling(True)
            zs, trace, _ = drc.record_run(p, self.x0, self.params)
            kt = p.kernel_times()
            p.set_kernel_profiling(False)
            got = (kt["k_frame_inv"][1], kt["k_schur"][1])
            _, cls = self.certify(family, p, zs, trace, self.mu0(p), kinds, what)
            assert got == drc.expected_launches(trace), (self.name, what, got, drc.expected_launches(trace), cls, [t["tries"] for t in trace])
        return zs, trace, cls


_RUNS = {}


def _run(name):
    if name not in _RUNS:
        _RUNS[name] = Run(name)
    return _RUNS[name]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# pass A instances, the epilogue in both forms
@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("wrench", [1, 0])
@pytest.mark.parametrize("variant", [641, 642, 644, 1284])
def test_pass_a_instances_invert_for_the_predicted_damping(variant, wrench, merge, monkeypatch):
    """k_passA<B, CPL, wrench> + k_passB (merge 0) and k_passAB<B, CPL, ..> (merge 1) on a set with frames of 2, 3, 10, 11, 12 slots beside
    full ones: the last lane of the last wavefront inverts, whatever the workgroup's shape"""
    _env(monkeypatch, AAR_PASSA_VARIANT=variant, AAR_PASSA_WRENCH=wrench, AAR_MERGE_PASSES=merge)
    r = _run("passa_cut")
    kf = dc.frame_entity_counts(r.ds)
    assert sorted(kf)[:5] == dc.SMALL_TARGETS and max(kf) > 20, kf
    r.run_one_gpu("pass A instances", what="variant %d wrench %d merge %d" % (variant, wrench, merge))


def test_merged_wrench_form_at_two_workgroups_per_cu(monkeypatch):
    """k_passAB_o2<B, CPL>"""
    _env(monkeypatch, AAR_PASSA_WRENCH=1, AAR_MERGE_PASSES=1, AAR_PASSAB_OCC2=1)
    _run("passa_cut").run_one_gpu("pass A instances", what="AAR_PASSAB_OCC2=1")


@pytest.mark.parametrize("name,lo,hi", [("avg_le_14", 0, 14), ("avg_15_30", 15, 30), ("avg_31_96", 31, 96), ("avg_gt_96", 96.001, 1e9)])
def test_pass_a_default_selection(name, lo, hi, monkeypatch):
    """no variant forced: <64, 1> up to 14 observations per frame, <64, 2> up to 30, <64, 4> up to 96, <128, 4> above (launch_passA_any)"""
    _env(monkeypatch)
    r = _run(name)
    avg = r.ds.num_obs / r.ds.num_frames
    assert lo <= avg <= hi and (name != "avg_15_30" or avg > 14), (name, avg)
    r.run_one_gpu("pass A instances", what="default selection, %.1f observations per frame" % avg)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# frames with more slots than a wavefront has lanes
@pytest.mark.parametrize("wrench", [1, 0])
@pytest.mark.parametrize("variant", [644, 1284])
def test_frames_with_more_slots_than_lanes(variant, wrench, monkeypatch):
    """up to 89 slots per frame: the wrench epilogue's ts != tid branch and the row form's strided copies"""
    _env(monkeypatch, AAR_PASSA_VARIANT=variant, AAR_PASSA_WRENCH=wrench)
    r = _run("wide_84")
    assert max(dc.frame_entity_counts(r.ds)) > 64
    r.run_one_gpu("wide frames", what="variant %d wrench %d" % (variant, wrench))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# dense panels from pass A (the MFMA Schur kernel): here AAR_DENSE_FROM_PASSA selects code
@pytest.mark.parametrize("wrench", [1, 0])
@pytest.mark.parametrize("F", [1, 2, 3, 5, 9])
@pytest.mark.parametrize("passa", [1, 0])
def test_dense_panels_short_frame_lists(passa, F, wrench, monkeypatch):
    _env(monkeypatch, AAR_SCHUR_MFMA=1, AAR_DENSE_FROM_PASSA=passa, AAR_PASSA_WRENCH=wrench)
    r = _run("mfma_F%d" % F)
    assert r.ds.num_frames == F and dc.tiles_of(r.ds) == 2
    r.run_one_gpu("dense panels", what="AAR_DENSE_FROM_PASSA=%d wrench %d" % (passa, wrench))


@pytest.mark.parametrize("passa", [1, 0])
@pytest.mark.parametrize("dense", [31, 32, 33])
def test_dense_panels_at_the_padding_boundary(dense, passa, monkeypatch):
    _env(monkeypatch, AAR_SCHUR_MFMA=1, AAR_DENSE_FROM_PASSA=passa)
    r = _run("dense_%d" % dense)
    assert dc.seen_entities(r.ds) + 1 == dense          # Ad = 32, 32, 64
    r.run_one_gpu("dense panels", what="dense count %d AAR_DENSE_FROM_PASSA=%d" % (dense, passa))


@pytest.mark.parametrize("wrench", [1, 0])
@pytest.mark.parametrize("passa", [1, 0])
def test_dense_panels_of_wide_frames(passa, wrench, monkeypatch):
    """more panel rows per frame (up to 6 x 89) than the workgroup has lanes: the panel loop strides"""
    _env(monkeypatch, AAR_SCHUR_MFMA=1, AAR_DENSE_FROM_PASSA=passa, AAR_PASSA_WRENCH=wrench)
    _run("wide_84").run_one_gpu("dense panels", what="wide frames AAR_DENSE_FROM_PASSA=%d wrench %d" % (passa, wrench))


@pytest.mark.parametrize("passa", [1, 0])
@pytest.mark.parametrize("split", [1, 100000])
def test_dense_panels_frame_pieces(split, passa, monkeypatch):
    _env(monkeypatch, AAR_SCHUR_MFMA=1, AAR_DENSE_FROM_PASSA=passa, AAR_SCHUR_SPLIT=split)
    _run("worklist_F60").run_one_gpu("dense panels", what="AAR_SCHUR_SPLIT=%d AAR_DENSE_FROM_PASSA=%d" % (split, passa))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# features
def test_huber_at_a_fixed_delta(monkeypatch):
    _env(monkeypatch)
    r = _run("huber")
    with r.problem() as p:
        assert p.get_huber_delta() == r.huber == 2.5
    r.run_one_gpu("features", what="Huber delta 2.5")


@pytest.mark.parametrize("merge", [1, 0])
@pytest.mark.parametrize("wrench", [1, 0])
def test_intrinsics(wrench, merge, monkeypatch):
    """k_passAB_intr<.., wrench> (merged) and k_passA_intr<.., wrench> + k_passB + k_passB_intr"""
    _env(monkeypatch, AAR_PASSA_WRENCH=wrench, AAR_MERGE_PASSES=merge)
    _run("intrinsics").run_one_gpu("features", what="intrinsics wrench %d merge %d" % (wrench, merge))


@pytest.mark.parametrize("merge", [1, 0])
def test_pose_priors_and_pair_priors(merge, monkeypatch):
    """k_prior and k_pair_prior sit between pass B and the speculative Schur complement (the device's H carries their blocks)"""
    _env(monkeypatch, AAR_MERGE_PASSES=merge)
    r = _run("priors")
    with r.problem() as p:
        assert p.n_priors == r.ds.num_cams - 1 and p.n_pair_priors == 6
    r.run_one_gpu("features", what="priors merge %d" % merge)


@pytest.mark.parametrize("which", ["fixed", "cams_off", "markers_off", "frames_off"])
def test_fixed_entities_and_groups_switched_off(which, monkeypatch):
    """frames_off is the frames_fixed branch of the epilogue: a zero inverse, no Schur terms, a step without a frame part"""
    _env(monkeypatch)
    r = _run(which)
    zs, trace, cls = r.run_one_gpu("features", what=which)
    if which == "fixed":
        for c in r.fixed["fixed_cams"]:
            col = slot_col(r.ds, "camera", c)
            assert all(np.array_equal(z[col:col + 6], zs[0][col:col + 6]) for z in zs)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# deterministic mode
@pytest.mark.parametrize("name", ["sweep1", "sweep3", "wide_84"])
def test_deterministic_runs_and_equal_bits(name, monkeypatch):
    """k_passA + k_passB_det + k_passB_reduce, k_schur<0, 1> + k_schur_reduce; wide_84 has more than 96 observations per frame: <64, 4> forced"""
    _env(monkeypatch)
    r = _run(name)
    if name == "wide_84":
        assert r.ds.num_obs / r.ds.num_frames > 96
    runs = []
    for _ in range(2):
        runs.append(r.run_one_gpu("deterministic", what="deterministic", deterministic=True))
    (za, ta, _), (zb, tb, _) = runs
    assert len(za) == len(zb) and all(np.array_equal(a, b) for a, b in zip(za, zb))
    assert [(t["mu"], t["err"], t["gain"]) for t in ta] == [(t["mu"], t["err"], t["gain"]) for t in tb]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# ranks through aar.LocalGroup
def _ranks_run(r, world):
    def solve(comm, rank):
        with r.problem(comm=comm) as q:
            zs, trace, _ = drc.record_run(q, r.x0, r.params)
            return zs, trace, q.local_obs
    return dc.run_ranks(world, solve)


def _certify_ranks(family, r, res, kinds, what):
    """every rank's recorded steps against the ONE-rank device H of the same problem (the ranks' sum differs from it in summation order only);
    the step callback hands every rank the whole gathered pose vector, so the frame part is certified on all frames"""
    with r.problem() as p:
        mu0 = r.mu0(p)
        done = []
        for rank, (zs, trace, _) in enumerate(res):
            same = [d for d in done if len(d[0]) == len(zs) and all(np.array_equal(a, b) for a, b in zip(d[0], zs))]
            if same:      # (the same bits as a rank already certified: the same certificate)
                assert [t["mu"] for t in trace] == [t["mu"] for t in same[0][1]]
                continue
            _, cls = r.certify(family, p, zs, trace, mu0, kinds, "%s rank %d" % (what, rank))
            done.append((zs, trace, cls))
    return done


@pytest.mark.parametrize("spec", [1, 0])
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("world,name", [(w, n) for w in (2, 3) for n in ("sweep2", "sweep5")])
def test_ranks(world, name, fused, spec, monkeypatch):
    """fused: the trial's S | rhs | g0 is all-reduced with the step's scalars (trial_reduced -> s_reduced), spec: the factorisation is queued too"""
    _env(monkeypatch, AAR_FUSED_COMM=fused, AAR_SPEC_CHOL=spec)
    r = _run(name)
    res = _ranks_run(r, world)
    assert all(x[2] > 0 for x in res), [x[2] for x in res]
    _certify_ranks("ranks", r, res, ("predicted",), "world %d fused %d spec %d" % (world, fused, spec))


def test_a_rank_without_frames(monkeypatch):
    _env(monkeypatch)
    r = _run("mfma_F2")
    res = _ranks_run(r, 3)
    assert min(x[2] for x in res) == 0 and r.ds.num_frames == 2, [x[2] for x in res]
    _certify_ranks("ranks", r, res, ("predicted",), "world 3, two frames")


@pytest.mark.parametrize("fused", [1, 0])
def test_ranks_after_a_step_with_a_small_gain(fused, monkeypatch):
    """an accepted step with gain < 0.94, then a one-try step: the reduced system was made for 0.33 mu -- with the fused collective it has been
    all-reduced already and cannot be taken back rank by rank: pass B alone rebuilds the rank's shared blocks (damped_try, s_reduced)"""
    _env(monkeypatch, AAR_FUSED_COMM=fused)
    r = _run("far_start")
    res = _ranks_run(r, 2)
    for zs, trace, cls in _certify_ranks("ranks, small gain", r, res, ("predicted", "taken back", "rebuilt"), "world 2 fused %d" % fused):
        assert any(c == "taken back" and trace[k - 1]["gain"] < 0.94 for k, c in enumerate(cls)), (cls, [t["gain"] for t in trace])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# repairs beside predictions in one run
def test_predicted_taken_back_and_rebuilt_steps_of_one_run(monkeypatch):
    """tau = 1e-6 from a far start: rejected tries (blocks rebuilt), accepted steps with gain < 0.94 (take-back + k_frame_inv) and predicted steps,
    one of them right behind a repair"""
    _env(monkeypatch)
    r = _run("far_start")
    zs, trace, cls = r.run_one_gpu("repairs", kinds=("predicted", "taken back", "rebuilt"), what="tau 1e-6")
    assert "rebuilt" in cls and "taken back" in cls, cls
    assert any(c == "predicted" and cls[k - 1] in ("rebuilt", "taken back") for k, c in enumerate(cls)), cls
