"""Certificates of the inexact reduced-system solves (SPCG: csrc/spcg_kernels.hip, PCG: csrc/pcg_kernels.hip) against a float64 restatement of the
same damped reduced system (tests/reduced_system.py, built from the oracle's dense normal equations).  Needs a real MI355X.

Every inexact solver promises a stopping rule (its header comment).  A step is checked against that rule on its own -- no trajectory, no final poses --
so a subtly wrong operator, preconditioner set-up or back-substitution fails here even where the LM gain test would still accept the step:

  PCG     |b - A32 d_s| <= 1.02 eta |b| with A32 the operator of the W blocks the solver holds (fp32 where it stores them so), and 1.05 eta against fp64 A;
          the solve stopped below its iteration cap, so the first conjunct of its rule is what held
  SPCG    block-Jacobi:  r^T D^-1 r <= (1.05 eta)^2 b^T D^-1 b          (D: the 6x6 diagonal blocks of A)
          coarse space:  r^T D^-1 r <= (1.05 eta)^2 (b^T D^-1 b + 2 b^T A^-1 b)  (the kernel's test is on the augmented system; for each group
                         b^T Z_g E_gg^-1 Z_g^T b <= b^T A^-1 b, so this bound holds without Z)
  every   the frame part is the back-substitution of the returned d_s: to 1e-10 against the solver's own W, 1e-6 against fp64 W; fixed entries exactly 0
  tight   at eta = 1e-12 with the coarse space forced on, the step is the exact float64 step (1e-7; SPCG 1e-6)

A try that SPCG gave up on (cap, flag 8) is redone by the direct chain (solver_stats()["fallbacks"]): such a step must meet the tight bar instead.
Steps are taken two ways: one-off (eval_damped_step at the start point and at points of a default LM run, mu from its trace) and the LM run's own
accepted steps (z from the step callback: the update is additive in z), which are the only ones where the coarse spaces join by themselves, k_pcgf keeps
its coarse operator between solves and the run's own forcing term applies.

Both a step from eval_damped_step and one from the callback are differences of two pose vectors: their rounding (an ulp of z) is allowed for explicitly.
"""
import threading

import numpy as np
import pytest

import aar
import oracle_lib as ol
from conftest import load_golden
from direct_run_certificate import mu_used as _mu_used
from reduced_system import ReducedSystem, held_mask, prior_terms, slot_col, split_indices

pytestmark = pytest.mark.gpu

PCG_ETA, SPCG_ETA = 5e-3, 3e-4          # kernels.h PCG_ETA_DEFAULT / SPCG_ETA_DEFAULT (the library's defaults; asserted through solver_stats)
SPCG_COARSE_FROM, PCG_COARSE_FROM = 12, 8
ULP = 2.3e-16                           # rounding of a difference of two pose vectors, relative to |z|


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class Case:
    """One problem: data set, the Problem's options, and the float64 reference built for it."""

    def __init__(self, ds, optimize=(True, True, True), with_huber=False, intrinsics=False, fixed_cams=(), fixed_markers=(), priors=None, **solver_kw):
        self.ds, self.optimize, self.huber, self.intr = ds, tuple(optimize), with_huber, intrinsics
        self.fixed_cams, self.fixed_markers, self.priors = list(fixed_cams), list(fixed_markers), priors
        self.kw = dict(optimize=optimize, with_huber=with_huber, intrinsics=intrinsics, **solver_kw)
        if fixed_cams or fixed_markers:
            self.kw.update(fixed_cams=list(fixed_cams), fixed_markers=list(fixed_markers))
        if priors:
            self.kw.update(priors=priors)
        self.ent, self.frames = split_indices(ds, optimize, intrinsics)

    def problem(self, **over):
        kw = dict(self.kw)
        kw.update(over)
        return aar.Problem(self.ds, **kw)

    def x0(self, p):
        return p.x_with_intrinsics(self.ds.x_full) if self.intr else np.asarray(self.ds.x_full, dtype=np.float64)

    def system(self, x, mu, huber_delta, w32=False, device_H=None):
        """the reduced system at x, mu: from the oracle's normal equations (+ the priors' numpy blocks), or from the device's own dense normal
        equations (device_H = (H, B): they carry the priors already) where the exact W bits the solver rounded are wanted"""
        ds = self.ds
        P = len(self.ent) + len(self.frames)
        held = held_mask(ds, P, self.fixed_cams, self.fixed_markers)
        if device_H is not None:
            H, B = device_H
            return ReducedSystem(H, B, mu, self.ent, self.frames, held=held, w32=w32)
        o = ol.Oracle(ds, optimize=self.optimize, with_huber=self.huber, huber_delta=huber_delta, intrinsics=self.intr)
        H, B = o.normal_equations(x, res_mode=ol.RES_F32)
        Hp = Bp = None
        if self.priors:
            Hp, Bp, _ = prior_terms(ds, x, self.priors, P)
        return ReducedSystem(H, B, mu, self.ent, self.frames, held=held, Hp=Hp, Bp=Bp, w32=w32)


def certify(rs, delta, z, solver, eta, coarse=False, fallback=False, iters=None, max_it=None, rs_own=None, what=""):
    """assert the solver's stopping rule and back-substitution for the step delta (z order) taken at the pose vector z.  rs: the float64 system
    (fp64 W); rs_own: the system with the W the solver holds (fp32-rounded for PCG with fp32 blocks; None: rs).  Returns a dict of the margins."""
    rs_own = rs if rs_own is None else rs_own
    ds_, df = rs.split(delta)
    zs, zf = rs.split(z)
    out = {}
    # fixed entities: exactly zero
    if rs.held_e.any():
        assert np.all(ds_[rs.held_e] == 0.0), what
    if len(ds_) == 0:
        return out
    # the rounding of z1 - z0: |A| ulp(z_s) on the residual
    nA = np.linalg.norm(rs.A64)          # (Frobenius: a bound of the 2-norm)
    slack = nA * ULP * np.linalg.norm(zs)
    if fallback:
        # redone by the direct chain: the exact step
        ex = rs.solve_s()
        assert np.linalg.norm(ds_ - ex) <= 1e-7 * np.linalg.norm(ex) + slack / max(np.linalg.eigvalsh(rs.A64)[0], 1e-300), (what, "fallback step")
    elif solver == "pcg":
        if iters is not None and max_it is not None:
            assert iters < max_it, (what, iters, max_it)
        nb = np.linalg.norm(rs_own.b)
        r_own = np.linalg.norm(rs_own.residual(ds_))
        r64 = np.linalg.norm(rs.residual(ds_, w32=False))
        out.update(pcg_own=r_own / nb, pcg_64=r64 / np.linalg.norm(rs.b64))
        assert r_own <= 1.02 * eta * nb + slack, (what, "|b - A32 d| / |b|", r_own / nb, eta)
        assert r64 <= 1.05 * eta * np.linalg.norm(rs.b64) + slack, (what, "|b - A d| / |b| (fp64 W)", r64 / np.linalg.norm(rs.b64), eta)
    elif solver == "spcg":
        rDr, bDb, bAb = rs.energy_norms(ds_)
        Dinv = rs.block_jacobi()
        dmax = max(np.abs(np.linalg.eigvalsh(Dinv[o:o + 6, o:o + 6])).max() for o in range(0, len(Dinv), 6))
        sl2 = dmax * slack ** 2
        lhs = np.sqrt(rDr)
        if coarse:
            bound = 1.05 * eta * np.sqrt(bDb + 2 * bAb)
            out.update(spcg_co=lhs / (eta * np.sqrt(bDb + 2 * bAb)), loose_ratio=(bDb + 2 * bAb) / bDb)
        else:
            bound = 1.05 * eta * np.sqrt(bDb)
            out.update(spcg_bj=lhs / (eta * np.sqrt(bDb)))
        assert lhs <= bound + np.sqrt(sl2), (what, "sqrt(r^T D^-1 r)", lhs, bound, "coarse" if coarse else "block-Jacobi")
    # back-substitution: against the solver's own W, and against fp64 W
    if rs.F:
        zsl = np.linalg.norm(zs) * ULP
        for sysm, tol, name in ((rs_own, 1e-10, "own W"), (rs, 1e-6, "fp64 W")):
            ref = sysm.backsub(ds_)
            scale = sysm.backsub_scale(ds_)
            # (rounding of z: ulp(z_f) and what ulp(z_s) becomes through V_f^-1 W_f^T)
            prop = np.linalg.norm(np.einsum("fij,efj->fie", sysm.Vinv, sysm.W32 if sysm.w32 else sysm.W64), axis=(1, 2)) * zsl
            err = np.linalg.norm(df - ref, axis=1)
            lim = tol * scale + ULP * np.linalg.norm(zf, axis=1) * 2 + prop * 2
            if sysm is rs and rs_own.w32:
                # (a solver with fp32 blocks against fp64 W: plus the fp32 rounding of W as it reaches the frame, V_f^-1 (W32 - W)^T d_s --
                #  measured 1.0e-6 .. 1.4e-6 of the scale on single frames of config-3 runs; against its own W the step is exact to 1e-10)
                lim = lim + 2 * np.linalg.norm(np.einsum("fij,fj->fi", rs.Vinv, np.einsum("efj,e->fj", rs.W32 - rs.W64, ds_)), axis=1)
            bad = np.nonzero(err > lim)[0]
            assert len(bad) == 0, (what, "back-substitution against " + name, bad[:5], (err[bad] / np.maximum(scale[bad], 1e-300))[:5])
    return out


def _one_off(case, p, x, mu, solver, eta, coarse, w32, what, ranks=False):
    st0 = p.solver_stats()
    d = p.eval_damped_step(x, mu)
    st1 = p.solver_stats()
    its = p.pcg_iterations()[0]
    hd = p.get_huber_delta() if case.huber else 10.0
    z = p.extract_z(x) + d     # (the pose the step ends at is z0 + delta, rounded; its size is what matters for the slack)
    rs = case.system(x, mu, hd)
    rs_own = None
    if w32:
        if ranks:
            rs_own = case.system(x, mu, hd, w32=True)
        else:
            H, B, _ = p.eval_normal_equations(x)
            rs_own = case.system(x, mu, hd, w32=True, device_H=(H, B))
    fb = st1["fallbacks"] > st0["fallbacks"]
    out = certify(rs, d, z, solver, eta, coarse=coarse, fallback=fb, iters=its, max_it=st1["pcg_max_it"] if solver == "pcg" else None,
                  rs_own=rs_own, what=what)
    return d, rs, out


def _lm_run(case, p, x0, every=4, max_checked=6):
    """a default LM run; returns (zs, per-step (iterations, fallbacks), trace, report)"""
    zs, info = [p.extract_z(x0)], []

    def cb(z):
        zs.append(z)
        info.append((p.pcg_iterations()[0], p.solver_stats()["fallbacks"]))

    p.set_step_callback(cb)
    x, rep = p.lm_solve(x0)
    p.set_step_callback(None)
    return zs, info, rep["trace"], rep


def _certify_run(case, p, x0, solver, eta, w32, coarse_possible, what, tau=1.0, n_check=5):
    hd = p.get_huber_delta() if case.huber else 10.0
    zs, info, trace, rep = _lm_run(case, p, x0)
    assert len(trace) >= 2 and all(t["accepted"] for t in trace[:-1])
    o = ol.Oracle(case.ds, optimize=case.optimize, with_huber=case.huber, huber_delta=hd, intrinsics=case.intr)
    # the trace's mu is the damping AFTER the step: the reference's rule max(1/3, 1 - (2 gain - 1)^3) applied to the damping of the accepted try.
    # mu0 (tau max diag J^T J) is read back from the first step, and checked against the oracle's diagonal where no prior adds to it
    fac = lambda t: max(0.33, 1 - (2 * t["gain"] - 1) ** 3)
    assert trace[0]["accepted"]
    mu0 = trace[0]["mu"] / fac(trace[0]) / _mu_used(trace, 0, 1.0)
    if not case.priors:
        H0, _ = o.normal_equations(x0, res_mode=ol.RES_F32)
        np.testing.assert_allclose(mu0, tau * float(np.diag(H0).max()), rtol=1e-9)
    for k, t in enumerate(trace):
        if t["accepted"] and k > 0:
            mu_k = _mu_used(trace, k, mu0)
            np.testing.assert_allclose(t["mu"], mu_k * fac(t), rtol=1e-9, err_msg="step %d" % k)
    # the run's first step is the one-off step at the start point with mu0 (a different damping -- e.g. the updated one -- moves it by tens of %)
    ks = sorted(set([0, 1, 2] + list(range(3, len(trace), max(1, len(trace) // n_check)))))
    ks = [k for k in ks if k < len(trace) and trace[k]["accepted"] and k + 1 < len(zs)][:n_check + 3]
    margins = []
    seen_big = False
    rejected_before = False
    for k in range(len(trace)):
        its, fbs = info[k]
        fb_prev = info[k - 1][1] if k else 0
        co = coarse_possible and (seen_big or rejected_before)
        if k in ks:
            mu = _mu_used(trace, k, mu0)
            x_k = o.merge_z(x0, zs[k])
            rs = case.system(x_k, mu, hd)
            rs_own = case.system(x_k, mu, hd, w32=True) if w32 else None
            d = zs[k + 1] - zs[k]
            m = certify(rs, d, zs[k + 1], solver, eta, coarse=co, fallback=fbs > fb_prev, iters=its,
                        max_it=p.solver_stats()["pcg_max_it"] if solver == "pcg" else None, rs_own=rs_own,
                        what="%s: LM step %d (mu %.3g, %d iterations)" % (what, k, mu, its))
            margins.append((k, its, m))
        if its >= (SPCG_COARSE_FROM if solver == "spcg" else PCG_COARSE_FROM):
            seen_big = True
        if trace[k]["tries"] > 1:
            rejected_before = True       # (a rejected try's count is never seen: it may have switched the coarse space on)
    return zs, trace, mu0, margins


# ---------------------------------------------------------------------------------------------------------------------------------------------
# SPCG: every k_spcg<nT, CO> instance, nT = 1 .. 14
def _spcg_ds(nT):
    # 16 nT - 3 entities (cameras + markers, roots included): the last tile is 13/16 full
    n = 16 * nT - 3
    C = 3 if nT == 1 else 4
    return aar.synth(2, num_cams=C, num_markers=n - C, num_frames=24, min_view_cos=0.01, seed=1000 + nT)


@pytest.mark.parametrize("spread", ["8", "1"])
@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("nT", list(range(1, 15)))
def test_spcg_steps_meet_the_stopping_rule_at_every_tile_count(nT, coarse, spread, monkeypatch):
    if spread == "1":
        monkeypatch.setenv("AAR_SPCG_SPREAD", "1")
    monkeypatch.setenv("AAR_SPCG_COARSE_FROM", "0" if coarse else "100000")
    ds = _spcg_ds(nT)
    case = Case(ds, solver="spcg")
    with case.problem() as p:
        st = p.solver_stats()
        assert st["solver"] == "spcg" and st["pcg_eta"] == SPCG_ETA
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, "spcg", SPCG_ETA, coarse, False, "nT %d coarse %s spread %s mu %.3g" % (nT, coarse, spread, mu))


@pytest.mark.parametrize("nT", [1, 3, 7, 14])
def test_spcg_tight_forcing_term_with_the_coarse_space_is_the_exact_step(nT, monkeypatch):
    # a preconditioner cannot change the solution; a wrong x = x' + Z c, Z^T b or augmented row can
    monkeypatch.setenv("AAR_SPCG_COARSE_FROM", "0")
    ds = _spcg_ds(nT)
    case = Case(ds, solver="spcg", pcg_eta=1e-12)
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()) * 1e-2, float(np.diag(H0).max()) * 1e-5):
            d = p.eval_damped_step(x, mu)
            ex = case.system(x, mu, 10.0).exact_step()
            assert _rel(d, ex) < 1e-6, (nT, mu, _rel(d, ex))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# PCG: every launched kernel (one rank)
PCG_VARIANTS = {
    "pcgf_w32_res": ({}, {}, True),                                         # k_pcgf<true, 1> (the default)
    "pcgf_w32": ({"AAR_PCG_RESIDENT": "0"}, {}, True),                      # k_pcgf<true>
    "pcgf_64_res": ({"AAR_PCG_W32": "0"}, {}, False),                       # k_pcgf<false, 2>
    "pcgf_64": ({"AAR_PCG_W32": "0", "AAR_PCG_RESIDENT": "0"}, {}, False),  # k_pcgf<false>
    "pcg_det": ({}, {"deterministic": True}, False),                        # k_pcg (fixed-order sums)
    "pcg_unfused": ({"AAR_PCG_FUSED": "0"}, {}, False),                     # k_pcg
}


def _cfg3_cut(frames=60):
    return aar.synth(3, num_frames=frames)


@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("variant", list(PCG_VARIANTS))
def test_pcg_steps_meet_the_stopping_rule_in_every_kernel(variant, coarse, monkeypatch):
    env, kw, w32 = PCG_VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0" if coarse else "100000")
    ds = _cfg3_cut()
    case = Case(ds, solver="pcg", **kw)
    with case.problem() as p:
        st = p.solver_stats()
        assert st["solver"] == "pcg" and st["pcg_eta"] == PCG_ETA
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, "pcg", PCG_ETA, coarse, w32, "%s coarse %s mu %.3g" % (variant, coarse, mu))


@pytest.mark.parametrize("variant", ["pcgf_w32_res", "pcgf_64_res", "pcg_det"])
def test_pcg_tight_forcing_term_with_the_coarse_space_is_the_exact_step(variant, monkeypatch):
    env, kw, _ = PCG_VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0")
    ds = _cfg3_cut()
    case = Case(ds, solver="pcg", pcg_eta=1e-12, pcg_max_it=2000, **kw)
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()) * 1e-2, float(np.diag(H0).max()) * 1e-5):
            d = p.eval_damped_step(x, mu)
            ex = case.system(x, mu, 10.0).exact_step()
            assert _rel(d, ex) < 1e-7, (variant, mu, _rel(d, ex))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The LM run's own steps (coarse spaces joining by themselves, the kept E of AAR_PCG_E_EVERY=3, the run's forcing term) and one-off steps at
# points inside the run
@pytest.mark.parametrize("solver,every", [("spcg", None), ("pcg", None), ("pcg", "3")])
def test_lm_run_steps_meet_the_stopping_rule(solver, every, monkeypatch):
    if every:
        monkeypatch.setenv("AAR_PCG_E_EVERY", every)
    ds = _cfg3_cut(100)
    case = Case(ds, solver=solver)
    eta = SPCG_ETA if solver == "spcg" else PCG_ETA
    with case.problem() as p:
        x0 = case.x0(p)
        zs, trace, mu0, margins = _certify_run(case, p, x0, solver, eta, solver == "pcg", solver == "spcg", "%s run" % solver)
        print("\n%s E_EVERY=%s: %d LM steps; margins %s" % (solver, every, len(trace), margins))
        # the first step against the one-off step at the start point with mu0
        d1 = p.eval_damped_step(x0, mu0)
        d_run = zs[1] - zs[0]
        assert np.linalg.norm(d_run - d1) <= 0.1 * np.linalg.norm(d1), np.linalg.norm(d_run - d1) / np.linalg.norm(d1)
        # one-off steps at late points of the run (small mu: the near-gauge modes make the CG work)
        o = ol.Oracle(ds)
        for k in (len(trace) // 2, len(trace) - 2):
            xk = o.merge_z(x0, zs[k + 1])
            _one_off(case, p, xk, trace[k]["mu"], solver, eta, False, solver == "pcg", "%s one-off at step %d" % (solver, k))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# PCG frame shapes: one, two and three 64-slot rounds; fewer frames than workgroups; empty frames; unobserved markers
def _frame_shapes_ds():
    # frame f keeps the observations of its first k_f - (its cameras) markers: 63 / 64 / 65 / 128 / 129 / 130 entities, one frame emptied; markers
    # 135 .. 139 are seen nowhere
    ds = aar.synth(2, num_cams=4, num_markers=140, num_frames=8, min_view_cos=0.01, seed=77)
    target = [64, 65, 66, 128, 129, 130, 0, 100]
    of, om, oc = np.asarray(ds.obs_frame), np.asarray(ds.obs_marker), np.asarray(ds.obs_cam)
    keep = np.zeros(ds.num_obs, bool)
    for f in range(ds.num_frames):
        sel = of == f
        ncam = len(set(oc[sel]))
        seen = sorted(set(om[sel & (om < 135)]))[:max(target[f] - ncam, 0)]
        keep |= sel & np.isin(om, seen)
    # (the root marker stays observed somewhere: it is marker 0 in every frame that keeps any)
    d2 = ds.select_observations(keep)
    kf = [len(set(np.asarray(d2.obs_marker)[np.asarray(d2.obs_frame) == f])) + len(set(np.asarray(d2.obs_cam)[np.asarray(d2.obs_frame) == f]))
          for f in range(d2.num_frames)]
    return d2, kf


@pytest.mark.parametrize("variant", ["pcgf_w32_res", "pcgf_64_res", "pcgf_w32", "pcg_det"])
def test_pcg_frame_shapes_of_one_two_and_three_rounds(variant, monkeypatch):
    env, kw, w32 = PCG_VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0")
    ds, kf = _frame_shapes_ds()
    assert {63, 64, 65, 128, 129, 130, 0} <= set(kf), kf
    case = Case(ds, solver="pcg", **kw)
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, "pcg", PCG_ETA, True, w32, "%s frame shapes mu %.3g" % (variant, mu))


@pytest.mark.parametrize("frames", [1, 5, 33])
@pytest.mark.parametrize("solver", ["pcg", "spcg"])
def test_few_frames_and_a_tail(frames, solver, monkeypatch):
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0")
    monkeypatch.setenv("AAR_SPCG_COARSE_FROM", "0")
    ds = aar.synth(2, num_cams=4, num_markers=30, num_frames=frames, min_view_cos=0.01, seed=5 + frames)
    case = Case(ds, solver=solver)
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, solver, PCG_ETA if solver == "pcg" else SPCG_ETA, True, solver == "pcg", "%d frames mu %.3g" % (frames, mu))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# camera counts: more than 64 (k_pcgf switches its coarse space off), a group with one non-root entity, a group with none
@pytest.mark.parametrize("name,kw", [("c66", dict(num_cams=66, num_markers=12, num_frames=30)),
                                     ("c2", dict(num_cams=2, num_markers=30, num_frames=40)),
                                     ("c1", dict(num_cams=1, num_markers=30, num_frames=40))])
@pytest.mark.parametrize("solver", ["pcg", "spcg"])
def test_camera_counts_with_the_coarse_space_forced_on(name, kw, solver, monkeypatch):
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0")
    monkeypatch.setenv("AAR_SPCG_COARSE_FROM", "0")
    ds = aar.synth(2, min_view_cos=0.01, seed=11, **kw)
    case = Case(ds, solver=solver)
    eta = PCG_ETA if solver == "pcg" else SPCG_ETA
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, solver, eta, True, solver == "pcg", "%s %s mu %.3g" % (name, solver, mu))


@pytest.mark.parametrize("solver", ["pcg", "spcg"])
def test_cameras_switched_off_with_the_coarse_space_forced_on(solver, monkeypatch):
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0")
    monkeypatch.setenv("AAR_SPCG_COARSE_FROM", "0")
    ds, _ = load_golden("g1_cfg3_cut")
    case = Case(ds, optimize=(False, True, True), solver=solver)
    eta = PCG_ETA if solver == "pcg" else SPCG_ETA
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, solver, eta, True, solver == "pcg", "cameras off %s mu %.3g" % (solver, mu))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# features: Huber weights, the intrinsics entities, fixed indices, pose priors (the coarse spaces are off with the last two)
def _priors(ds, x, seed=3):
    rng = np.random.default_rng(seed)
    pr = []
    for c in range(ds.num_cams):
        if c != ds.root_cam:
            col = slot_col(ds, "camera", c)
            A = rng.standard_normal((6, 6))
            pr.append(("camera", c, x[col:col + 6] + np.r_[0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)], 1e3 * (A @ A.T + 6 * np.eye(6))))
    return pr


def _feature_case(feature, solver):
    ds, _ = load_golden("g1_cfg2_huber" if feature == "huber" else ("g1_cfg2_intr" if feature == "intrinsics" else "g1_cfg3_cut"))
    if feature == "huber":
        return Case(ds, with_huber=True, solver=solver)
    if feature == "intrinsics":
        return Case(ds, intrinsics=True, solver=solver)
    if feature == "fixed":
        fc = [c for c in range(ds.num_cams) if c != ds.root_cam][:2]
        fm = [m for m in range(ds.num_markers) if m != ds.root_marker][1:4]
        return Case(ds, fixed_cams=fc + [ds.root_cam], fixed_markers=fm, solver=solver)
    return Case(ds, priors=_priors(ds, ds.x_full), solver=solver)


@pytest.mark.parametrize("feature,solver", [("huber", "spcg"), ("huber", "pcg"), ("intrinsics", "spcg"), ("fixed", "spcg"), ("fixed", "pcg"),
                                            ("priors", "spcg"), ("priors", "pcg")])
def test_feature_steps_meet_the_stopping_rule(feature, solver):
    case = _feature_case(feature, solver)
    eta = PCG_ETA if solver == "pcg" else SPCG_ETA
    with case.problem() as p:
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, solver, eta, False, solver == "pcg", "%s %s mu %.3g" % (feature, solver, mu))
        if feature in ("huber", "priors", "fixed"):
            _certify_run(case, p, x, solver, eta, solver == "pcg", solver == "spcg" and feature == "huber", "%s %s run" % (feature, solver), n_check=3)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# PCG with the frames sharded over in-process ranks: k_pcgd_iter_f<true / false>, k_pcgd_iter; one rank without frames
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


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("variant", ["pcgf_w32_res", "pcgf_64_res", "pcg_det"])
def test_sharded_pcg_steps_meet_the_stopping_rule(variant, world, monkeypatch):
    env, kw, w32 = PCG_VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AAR_PCG_COARSE_FROM", "0")
    # world 3: two frames only -- the third rank gets none
    ds = _cfg3_cut(60) if world == 2 else aar.synth(3, num_frames=2)
    case = Case(ds, solver="pcg", **kw)
    o = ol.Oracle(ds)
    H0, _ = o.normal_equations(ds.x_full, res_mode=ol.RES_F32)
    mus = (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4)

    def solve(comm, rank):
        with aar.Problem(ds, comm=comm, solver="pcg", **kw) as q:
            st = q.solver_stats()
            return [(q.eval_damped_step(ds.x_full, mu), q.pcg_iterations()[0], st["pcg_max_it"], q.local_obs) for mu in mus]
    res = _run_ranks(world, solve)
    if world == 3:
        assert min(r[0][3] for r in res) == 0, [r[0][3] for r in res]
    for i, mu in enumerate(mus):
        d0 = res[0][i][0]
        for r in range(world):
            assert _rel(res[r][i][0], d0) < 1e-12          # (every rank returns the same gathered step)
        rs = case.system(ds.x_full, mu, 10.0)
        rs_own = case.system(ds.x_full, mu, 10.0, w32=True) if w32 else None
        certify(rs, d0, o.extract_z(ds.x_full) + d0, "pcg", PCG_ETA, iters=res[0][i][1], max_it=res[0][i][2], rs_own=rs_own,
                what="%s world %d mu %.3g" % (variant, world, mu))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# AUTO at its defaults
@pytest.mark.parametrize("shape", ["cfg3_cut", "cfg5_shaped"])
def test_auto_picks_and_its_step_meets_the_stopping_rule(shape):
    ds = aar.synth(3, num_frames=100) if shape == "cfg3_cut" else aar.synth(5, num_frames=400)
    want = "spcg" if shape == "cfg3_cut" else "pcg"
    case = Case(ds)
    with case.problem() as p:
        st = p.solver_stats()
        assert st["solver"] == want, st
        eta = SPCG_ETA if want == "spcg" else PCG_ETA
        assert st["pcg_eta"] == eta
        x = case.x0(p)
        H0, _, _ = p.eval_normal_equations(x)
        for mu in (float(np.diag(H0).max()), float(np.diag(H0).max()) * 1e-4):
            _one_off(case, p, x, mu, want, eta, False, want == "pcg", "AUTO %s mu %.3g" % (shape, mu))
