"""The observation passes on the device -- k_unpack (make_ent_row), k_residual, pass A (V_f, g_f, W), pass B (U, g), alone or merged --
against tests/projection_reference.py: a float64 restatement of the FORWARD model differentiated by the complex step, which shares no
formula with csrc/geom.hpp (no closed-form Jacobian, no left Jacobian of SO(3), no series switch at 1e-2).  tests/test_projection_reference_host.py
checks that reference against mpmath (4e-16) and the oracle against it on the CPU; this file asks the DEVICE, in every branch of make_ent_row
and every kernel instance the launchers of csrc/eval_kernels.hip can pick.

Everything goes through Problem.eval_residuals / eval_normal_equations / eval_damped_step with solver="direct".  Bars (the project's own,
tests/test_gpu_parity.py): H 1e-12 of max|H|, B 1e-11 of max|B|, residual rows 1e-9 px in double mode, damped step 1e-8 of max|delta| against
numpy.linalg.solve(H_ref + mu I, B_ref); and the diagonal-scaled measure |H - H_ref|_ij / sqrt(H_ii H_jj) below projection_reference.SCALED_BAR
(5e-12 = 100 x the oracle's worst on the CPU).  Float mode without Huber: rows bit-equal to the reference (the host file shows the reference
bit-equal to the oracle there on every input); Huber rows in float mode differ from the reference by one rounding on the CPU already, so
their bit-equality stays with the oracle (tests/test_gpu_parity.py) and here they are held to 1e-9 px.
mu = 1e-2 max diag(H_ref): the device's H agrees with the reference to ~1e-13 of max|H| (summation order), a damped system of condition
<= ~1e4 turns that into <= 1e-9 of the step -- ten times inside the bar, so the step test sees the blocks and not the conditioning.

Which kernel instance each combination launches (launch_passA_t<B, CPL> picks among k_passA / k_passA_intr / k_passAB / k_passAB_o2 /
k_passAB_intr; launch_passB among k_passB<wrench> / k_passB_det + k_passB_reduce / k_passB_intr /
k_passB_intr_det) is listed in the docstring of the test that reaches it.  The launch counts of kernel_times tell a merged launch from
separate ones; they do not tell WHICH template instance ran (all of pass A's share one counter), so a switch the launcher ignores is seen
only through the docstrings' reading of launch_passA_any / launch_passA_t: AAR_PASSA_VARIANT is ignored in deterministic mode above 96
observations per frame, AAR_PASSAB_OCC2 with intrinsics.

NOT covered here: what pass A writes for the NEXT solve -- (V_f + mu I)^-1 and h_f, and with the MFMA Schur kernel the dense panels W,
Y = W (V_f + mu I)^-1 (passA_epilogue and its wrench twin).  It is written only when the LM loop evaluates a trial point with a predicted
damping; eval_normal_equations and eval_damped_step never ask for it (their panels come from k_schur_fill, their inverses from k_frame_inv),
so AAR_DENSE_FROM_PASSA makes no difference to them and is not part of any matrix below.  That epilogue is certified where it runs, inside
LM runs, in every workgroup shape: tests/test_gpu_speculative_path.py (and, at the default shape of their fixtures, pinned by the LM traces
of tests/test_gpu_parity.py against the oracle and the real solver).

MEASURED on an MI355X (largest over each test's combinations; H and B relative to max|H_ref|, max|B_ref|):
  edge poses (25 data sets x 20 problems):  H 4.2e-15 (theta = 0.01 + 1e-6; elsewhere <= 1.7e-15), B 2.2e-13 (double mode), rows 4.6e-13 px,
                                            damped step 2.5e-11, scaled measure 9.5e-13 (deterministic, the -board sets; others 2.6e-13 .. 7.7e-13)
  other chart (g1_cfg2 + 2 pi):             H 6.5e-16, B 4.8e-15, rows 6.8e-13 px, step 1.0e-12, scaled 5.5e-15
  pass A shapes (51 + 41 problems):         H 1.0e-15, B 3.6e-14, rows 4.6e-13 px, step 1.4e-11, scaled 1.03e-12 (wrench form, separate launches)
  pass B chunks (4 modes, 24 each):         H 9.4e-16, B 5.1e-14, rows 3.4e-13 px, step 3.3e-11 (intrinsics), scaled 9.95e-13
  both passes, P = 6642, chunks of 512:     H 1.6e-15, B 1.6e-14, rows 2.3e-13 px, scaled 5.2e-13
  config 5, 1.26 M observations, frames off: H 2.3e-15, B 1.4e-14, rows 1.0e-12 px, step 5.0e-14, scaled 9.9e-13
  config 5, first 200 frames:               H 2.1e-15, B 1.4e-14, rows 9.1e-13 px, step 5.9e-14, scaled 2.8e-15
  The scaled measure is the one figure near its bar (5x inside): ~1e-12 wherever pass A or B runs in wrench form, whose 6 x 6 images carry
  lever arms of ~3 units; the oracle's row form gives 5e-14 at worst on the CPU.
  Float-mode rows without Huber were bit-equal to the reference in every case.  Wall time of the file: 45 s, of which
  test_config5_shared_blocks_at_full_size takes 26 s (aar.synth(5) and the reference streamed over 1.26 M observations), the 200-frame slice 2.7 s,
  the two pass A matrices 1.6 s each, and every other test under 1.4 s.
"""
import numpy as np
import pytest

import aar
import projection_reference as pr
from conftest import load_golden

pytestmark = pytest.mark.gpu

H_BAR, B_BAR, ROW_BAR, STEP_BAR = 1e-12, 1e-11, 1e-9, 1e-8
ALL, FRAMES_ONLY, SHARED_ONLY = (True, True, True), (False, False, True), (True, True, False)
PASSA_ENV = ("AAR_PASSA_VARIANT", "AAR_PASSA_WRENCH", "AAR_MERGE_PASSES", "AAR_PASSAB_OCC2", "AAR_SCHUR_MFMA",
             "AAR_DENSE_FROM_PASSA", "AAR_PASSB_CHUNK")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


class Ref:
    """reference results of one data set, computed once per (switches, residual mode)"""

    def __init__(self, ds, x_pose=None):
        self.ds, self.x, self.cache = ds, (ds.x_full if x_pose is None else x_pose), {}

    def get(self, optimize, intrinsics, huber, res):
        key = (optimize, intrinsics, huber, res)
        if key not in self.cache:
            R = pr.Reference(self.ds, optimize=optimize, intrinsics=intrinsics, huber_delta=huber)
            H, B, ss = R.normal_equations(self.x, res)
            self.cache[key] = (R, H, B, ss, R.residuals(self.x, res))
        return self.cache[key]


def _set_env(monkeypatch, **env):
    for k in PASSA_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, str(v))


def _compare(ref, worst, tag, optimize=ALL, intrinsics=False, huber=None, res=aar.RES_F64, det=False, step=True, rows=True, profile=False):
    """one Problem against the reference: rows, H, B, ss, the scaled measure and a damped step; returns the launch counts when profile"""
    ds = ref.ds
    R, Hr, Br, ssr, rr = ref.get(optimize, intrinsics, huber, res)
    counts = None
    with aar.Problem(ds, residual_mode=res, optimize=optimize, with_huber=huber is not None, intrinsics=intrinsics, solver="direct",
                     deterministic=det) as p:
        if huber is not None:
            p.set_huber_delta(huber)
        assert p.num_vars == R.P
        x = p.x_with_intrinsics(ref.x) if intrinsics else ref.x
        fig = {}
        if rows:
            r, ss = p.eval_residuals(x)
            fig["rows"] = float(np.abs(r - rr).max())
            if res == aar.RES_F32 and huber is None:
                assert np.array_equal(r, rr), (tag, "float-faithful rows differ from the reference")
            assert abs(ss - ssr) <= 1e-12 * ssr, (tag, ss, ssr)
        if profile:
            p.set_kernel_profiling(True)
        H, B, ss = p.eval_normal_equations(x)
        if profile:
            kt = p.kernel_times()
            counts = (kt["k_passA"][1], kt["k_passB"][1])
            p.set_kernel_profiling(False)
        fig["H"] = float(np.abs(H - Hr).max() / np.abs(Hr).max())
        fig["B"] = float(np.abs(B - Br).max() / np.abs(Br).max())
        fig["scaled"] = pr.scaled_error(H, Hr)
        fig["ss"] = abs(ss - ssr) / ssr
        if intrinsics:
            i0 = R.z_intr0
            assert not H[i0:, :].reshape(-1, 9, R.P)[:, 4:, :].any() and not H[:, i0:].reshape(R.P, -1, 9)[:, :, 4:].any()
        if step:
            mu = 1e-2 * float(np.diag(Hr).max())
            d = p.eval_damped_step(x, mu)
            dr = np.linalg.solve(Hr + mu * np.eye(R.P), Br)
            fig["step"] = float(np.abs(d - dr).max() / np.abs(dr).max())
    for k, v in fig.items():
        if v > worst.get(k, (-1.0, None))[0]:
            worst[k] = (v, tag)
    print("%s: %s" % (tag, " ".join("%s %.2e" % kv for kv in sorted(fig.items()))))
    assert np.abs(H - H.T).max() == 0.0, tag
    assert fig["H"] < H_BAR and fig["B"] < B_BAR and fig["scaled"] < pr.SCALED_BAR and fig["ss"] < 1e-12, (tag, fig)
    assert fig.get("rows", 0.0) < ROW_BAR and fig.get("step", 0.0) < STEP_BAR, (tag, fig)
    return counts


def _report(name, worst):
    print("WORST %s: %s" % (name, "; ".join("%s %.2e (%s)" % (k, v[0], v[1]) for k, v in sorted(worst.items()))))


# ------------------------------------------------------------------------------------------------ a. edge poses
EDGE_CASES = [(th, board, False) for th in pr.EDGE_ANGLES for board in (False, True)] + [(0.0, False, True)]


def _edge_id(case):
    return "theta=%.17g%s%s" % (case[0], "-board" if case[1] else "", "-t0" if case[2] else "")


@pytest.mark.parametrize("case", EDGE_CASES, ids=_edge_id)
def test_edge_poses(case, monkeypatch):
    """make_ent_row's branches on the device: theta given to camera 1, marker 1 and frame 1 at once (-board: to every marker; -t0: with zero
    translation too).  exactly 0, 1e-20, 1e-17: R = I (th < DBL_EPSILON) while J_l takes its series; 3e-16 .. 0.01 - 1e-6: Rodrigues in closed
    form, J_l by series; 0.01 + 1e-6 and up: both in closed form; pi -+ 1e-9, pi; 2 pi - 1e-3 where J_l is close to losing rank.
    Both residual modes x Huber off / on (delta = 1.5 px: ~30 % of the corners beyond it, and one corner with e = 0 exactly in float mode) x
    intrinsics off / on x deterministic off / on, and each group switched off in turn.  Small problems, default switches: the merged launch
    k_passAB<64, 2 or 4, wrench, row-form B> (k_passAB_intr with intrinsics), deterministic: k_passA + k_passB_det + k_passB_reduce
    (+ k_passB_intr_det)."""
    _set_env(monkeypatch)
    ds = pr.edge_dataset(case[0], board=case[1], zero_translation=case[2])
    ref, worst = Ref(ds), {}
    R, _, _, _, rr = ref.get(ALL, False, 1.5, aar.RES_F32)
    raw = pr.Reference(ds).residuals(ds.x_full, pr.RES_F32).reshape(-1, 2)
    e = (raw ** 2).sum(axis=1)
    assert e[0] == 0.0 and (e > 1.5 ** 2).sum() > 10 and ((e > 0) & (e <= 1.5 ** 2)).sum() > 10     # all three branches of the weight occur
    for res in (aar.RES_F64, aar.RES_F32):
        for huber in (None, 1.5):
            for intr in (False, True):
                for det in (False, True):
                    _compare(ref, worst, "res=%d huber=%s intr=%d det=%d" % (res, huber, intr, det), intrinsics=intr, huber=huber, res=res, det=det)
    for opt in ((False, True, True), (True, False, True), SHARED_ONLY, FRAMES_ONLY):
        _compare(ref, worst, "optimize=%s" % (opt,), optimize=opt)
    _report(_edge_id(case), worst)


def test_other_chart_and_the_series_switch(monkeypatch):
    """theta + 2 pi for g1_cfg2's own theta on two cameras, two markers and two frames: the same rotations in another chart -- device and
    reference must agree in THAT chart.  And H is continuous across |w| = 1e-2 to the bar: the device's H moves from 0.01 - 1e-6 to
    0.01 + 1e-6 by what the reference's moves."""
    _set_env(monkeypatch)
    ds, _ = load_golden("g1_cfg2")
    C, M = ds.num_cams, ds.num_markers
    x = pr.other_chart(ds.x_full, [0, 2, C - 1, C - 1 + 3, C - 1 + M - 1, C - 1 + M - 1 + 5])
    ref, worst = Ref(ds, x), {}
    for res in (aar.RES_F64, aar.RES_F32):
        for intr in (False, True):
            _compare(ref, worst, "other chart res=%d intr=%d" % (res, intr), intrinsics=intr, res=res)
    _report("other chart", worst)
    jump_dev, jump_ref = [], []
    for th in (0.01 - 1e-6, 0.01 + 1e-6):
        ds = pr.edge_dataset(th)
        jump_ref.append(pr.Reference(ds).normal_equations(ds.x_full)[0])
        with aar.Problem(ds, residual_mode=aar.RES_F64, solver="direct") as p:
            jump_dev.append(p.eval_normal_equations(ds.x_full)[0])
    scale = np.abs(jump_ref[0]).max()
    cont = np.abs((jump_dev[1] - jump_dev[0]) - (jump_ref[1] - jump_ref[0])).max() / scale
    print("series switch: |dH| %.2e of max|H|, device - reference %.2e" % (np.abs(jump_ref[1] - jump_ref[0]).max() / scale, cont))
    assert np.abs(jump_ref[1] - jump_ref[0]).max() / scale < 1e-3 and cont < H_BAR


# ------------------------------------------------------------------------------------------------ b. pass A shapes
FRAME_COUNTS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320]   # 320 = 8 x 40: every camera and marker in one frame
VARIANTS = {None: "<128, 4> (100.6 observations per frame on average: above 96)", 641: "<64, 1>", 642: "<64, 2>", 644: "<64, 4>",
            1284: "<128, 4>"}


@pytest.mark.parametrize("intrinsics", [False, True], ids=["poses", "intrinsics"])
def test_pass_a_workgroup_shapes(intrinsics, monkeypatch):
    """One data set whose 18 frames carry 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 320 observations
    (max_kf from 2 entities up to all 8 cameras + 40 markers in one frame; 1811 / 18 = 100.6 per frame, so the size rule itself picks
    launch_passA_t<128, 4>), under

      AAR_PASSA_VARIANT unset -> <128, 4>, 641 -> <64, 1>, 642 -> <64, 2>, 644 -> <64, 4>, 1284 -> <128, 4>                   (launch_passA_any)
      x AAR_PASSA_WRENCH 1 / 0                                                               (the WR template argument: wrench form / row form)
      x AAR_MERGE_PASSES 1 / 0 with all groups on:
          merged, poses:      k_passAB<B, CPL, true> (wrench A, row-form B: the default), k_passAB<B, CPL, false> (row form)
          merged, intrinsics: k_passAB_intr<B, CPL, true / false>
          separate:           k_passA<B, CPL, true / false> or k_passA_intr<..>, then k_passB<true / false> (+ k_passB_intr)
        asserted from the launch counts of set_kernel_profiling / kernel_times: merged -> no k_passB launch, separate -> both
      x frames-only problems (optimize = (False, False, True)): H is exactly pass A's V_f, B its g_f
    plus, merged and in wrench form: AAR_PASSAB_OCC2=1 -> k_passAB_o2<B, CPL>, AAR_PASSAB_OCC2=0 -> k_passAB<B, CPL, true>
    (poses only: with intrinsics both launch the same k_passAB_intr<B, CPL, true>, so they are not repeated there).
    With AAR_SCHUR_MFMA=1 the one-off entry points run k_schur_fill + the MFMA Schur kernel behind eval_damped_step (per variant and form);
    pass A's own panel writer is not reached that way (see the module docstring)."""
    ds = pr.frame_counts_dataset(FRAME_COUNTS)
    ref, worst = Ref(ds), {}
    for variant in VARIANTS:
        for wrench in (1, 0):
            for merge in (1, 0):
                _set_env(monkeypatch, AAR_PASSA_VARIANT=variant, AAR_PASSA_WRENCH=wrench, AAR_MERGE_PASSES=merge)
                tag = "variant=%s wrench=%d merge=%d" % (variant, wrench, merge)
                nA, nB = _compare(ref, worst, tag + " all", intrinsics=intrinsics, profile=True, rows=False)
                assert nA >= 1 and (nB == 0 if merge else nB >= 1), (tag, nA, nB)      # merged: pass B's chunks rode in pass A's launch
                if merge:       # (frames only: nothing of pass B reaches H; one launch form is enough)
                    _compare(ref, worst, tag + " frames-only", optimize=FRAMES_ONLY, intrinsics=intrinsics, rows=False)
        for extra in (() if intrinsics else (dict(AAR_PASSAB_OCC2=1), dict(AAR_PASSAB_OCC2=0))):
            _set_env(monkeypatch, AAR_PASSA_VARIANT=variant, AAR_PASSA_WRENCH=1, AAR_MERGE_PASSES=1, **extra)
            nA, nB = _compare(ref, worst, "variant=%s %s" % (variant, extra), intrinsics=intrinsics, profile=True, rows=False)
            assert nA >= 1 and nB == 0
        for wrench in (1, 0):
            _set_env(monkeypatch, AAR_PASSA_VARIANT=variant, AAR_PASSA_WRENCH=wrench, AAR_SCHUR_MFMA=1)
            _compare(ref, worst, "variant=%s wrench=%d mfma one-off" % (variant, wrench), intrinsics=intrinsics, rows=False)
    _set_env(monkeypatch)
    _compare(ref, worst, "deterministic", intrinsics=intrinsics, det=True)     # avg > 96 and deterministic: <64, 4>, one wavefront per frame
    _report("pass A shapes, intrinsics=%s" % intrinsics, worst)


# ------------------------------------------------------------------------------------------------ c. pass B chunks
RUN_LENGTHS = [63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049]
CHUNKS = [None, 64, 128, 256, 512, 1024]


@pytest.mark.parametrize("mode", ["atomic", "deterministic", "intrinsics", "intrinsics_deterministic"])
def test_pass_b_chunks(mode, monkeypatch):
    """Frames switched off (optimize = (True, True, False)): H is exactly pass B's U and B its g, and P stays 42 (69 with intrinsics) while the
    13 (camera, marker) runs are 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025 and 2049 observations long (N = 7233, 2049 frames).
    AAR_PASSB_CHUNK unset (64: N < 131 072) / 64 / 128 / 256 / 512 / 1024: 1 .. 16 observations per lane, runs that end one short of, at and
    one past a chunk's end.
      atomic, AAR_MERGE_PASSES=0:  k_passB<true> (wrench), k_passB<false> (AAR_PASSA_WRENCH=0)
      atomic, merged (default):    the chunks ride in k_passAB<64, 1, true> (7233 / 2049 = 3.5 observations per frame: <64, 1>);
                                   AAR_PASSA_WRENCH=0 -> k_passAB<64, 1, false>
      deterministic:               k_passB_det<true / false> + k_passB_reduce (never merged)
      intrinsics:                  separate k_passB<..> + k_passB_intr; merged k_passAB_intr<64, 1, ..>
      intrinsics_deterministic:    k_passB_det + k_passB_intr_det + k_passB_reduce
    The launch counts (kernel_times) say which path ran."""
    det, intr = "deterministic" in mode, "intrinsics" in mode
    ds = pr.run_lengths_dataset(RUN_LENGTHS)
    ref, worst = Ref(ds), {}
    for chunk in CHUNKS:
        for merge in (1, 0):
            for wrench in (1, 0):
                _set_env(monkeypatch, AAR_PASSB_CHUNK=chunk, AAR_MERGE_PASSES=merge, AAR_PASSA_WRENCH=wrench)
                tag = "%s chunk=%s merge=%d wrench=%d" % (mode, chunk, merge, wrench)
                nA, nB = _compare(ref, worst, tag, optimize=SHARED_ONLY, intrinsics=intr, det=det, profile=True, rows=(chunk is None and merge == 1 and wrench == 1))
                merged = merge == 1 and not det
                assert nA >= 1 and (nB == 0 if merged else nB >= 1), (tag, nA, nB)
    _report("pass B chunks, " + mode, worst)


def test_passes_tied_together_at_a_long_chunk(monkeypatch):
    """All groups on, 1100 frames, runs up to 1025 observations, AAR_PASSB_CHUNK=512: P = 6642 (a dense H of 353 MB: this one case only).
    Pass A (k_passA<64, 1, true>) and pass B (k_passB<true>, up to 8 observations per lane) as launches of their own, and the same merged
    (k_passAB<64, 1, true>)."""
    ds = pr.run_lengths_dataset(RUN_LENGTHS[:-1], F=1100)
    ref, worst = Ref(ds), {}
    for merge in (0, 1):
        _set_env(monkeypatch, AAR_PASSB_CHUNK=512, AAR_MERGE_PASSES=merge)
        nA, nB = _compare(ref, worst, "P=6642 chunk=512 merge=%d" % merge, profile=True, step=False, rows=(merge == 0))
        assert nA >= 1 and (nB == 0 if merge else nB >= 1)
    _report("passes tied together", worst)


# ------------------------------------------------------------------------------------------------ d. config 5 at full size
def test_config5_shared_blocks_at_full_size(monkeypatch):
    """aar.synth(5), default switches (chunks of 512, pass B as a launch of its own: k_passB<true>), frames switched off: P = 6 x 214, so
    U and g of all 1.26 M observations come back dense, and the reference streams the observations in slices of 16 384.  Double mode."""
    _set_env(monkeypatch)
    ds = aar.synth(5)
    ref, worst = Ref(ds), {}
    nA, nB = _compare(ref, worst, "config 5, frames off", optimize=SHARED_ONLY, profile=True)
    assert nB >= 1                                           # (too many wavefronts to merge: pass B ran as its own launch)
    _report("config 5 shared blocks", worst)


def test_config5_frame_blocks_on_a_slice(monkeypatch):
    """Pass A's workgroups are independent per frame: the first 200 frames of config 5 (~250 observations per frame: launch_passA_t<128, 4>,
    two wavefronts per frame) with only the frames on stand for the 5000; then all groups on, merged or not as the launcher decides, against
    the dense reference (P = 2484) (216 shared entities: the MFMA Schur kernel, its panels from k_schur_fill, behind the damped step)."""
    _set_env(monkeypatch)
    ds = pr.cut_frames(aar.synth(5), 200)
    ref, worst = Ref(ds), {}
    _compare(ref, worst, "config 5 / 200 frames, frames only", optimize=FRAMES_ONLY)
    _compare(ref, worst, "config 5 / 200 frames, all groups", rows=False)
    _report("config 5 frame blocks", worst)
