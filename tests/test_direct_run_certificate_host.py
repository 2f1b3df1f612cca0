"""The run certificate of the direct chain (tests/direct_run_certificate.py) on the host: every run that tests/test_gpu_speculative_path.py takes
on the device offers its predicted steps, plain float64 stays inside the bar on them, and a step made from a WRONG speculation does not.
H, B come from the oracle; no GPU.

The LM rule of aar_lm_step is restated in numpy on the oracle's normal equations (host_lm): the step is rs.solve_s() + rs.backsub(), the gain
(err - prev) / (0.5 (mu |d|^2 - d.g)), accepted when gain > 0 and the error fell, mu *= max(0.33, 1 - (2 gain - 1)^3) and v = 2 then, mu *= v and
v *= 5 otherwise, six tries at the most, the stop rule of aar_lm_solve with the default parameters, ten steps.  (0.5 (mu |d|^2 - d.g) is minus HALF
the decrease the linear model predicts for sum r^2, so a step in the linear regime has gain >= 2 and is followed by 0.33 mu: the predicted step
is the common one.  Gains below 0.94 need a start far from the solution: direct_cases.far_start_ds with tau = 1e-6.)

Premise, per run of direct_cases.SPEC_RUNS (data set, options, tau): at least its stated number of predicted steps among the first ten.  Measured:
nine of ten steps are predicted in every run with tau = 1 (gains 2.9 .. 12.3; Huber at delta 2.5: 1.05 .. 3.5); far_start (tau = 1e-6) gives
first, 3 predicted, rebuilt (3 tries, gain 0.72), taken back (gain 0.52), taken back, 2 rebuilt, predicted -- four predicted, the last behind a repair.

Reference within the bar: the float64 step of every certified step of those runs (the first six predicted ones; in far_start the taken-back and
rebuilt ones too) -- d itself, as tests/test_direct_certificate_host.py takes its reference, with a frame part by np.linalg.solve on V_f -- stays
at ratio <= 1/8 in (a) and (c).  The same step read back as zs[k + 1] - zs[k], rounded through z like the device's, must pass the certificate;
its ratio is the rounding of z that the slack term allows for (a bound: up to 1/2 where few large entries of z carry a block row, as the
focal lengths and principal points of an intrinsics entity do), so it is recorded, not held to 1/8.  Worst measured per family:
                                                              the step itself             read back as z1 - z0
                                                              |r| / bar    frame part     |r| / bar    frame part
    pass A sets (cut frames, four averages, wide, 60 frames)  9.3e-4       1.1e-5         5.0e-2       9.3e-3
    MFMA frame lists, dense counts                            8.0e-4       4.9e-5         3.6e-2       1.9e-3
    features (Huber, intrinsics, priors, fixed, groups off)   6.1e-4       3.7e-5         1.44e-1      7.4e-3      (intrinsics; the others <= 3.4e-2)
    tile sweep 1, 2, 3, 5, 7                                  9.6e-4       1.5e-5         5.0e-2       2.3e-3
    far start (tau = 1e-6)                                    8.6e-9       1.0e-2         7.2e-8       1.1e-3
(far start: at mu = 1e-6 max diag H the frame blocks' kappa_f is ~1e6 and weights the bar of (a) accordingly: there part (a) resolves little and
part (c), whose bar does not carry kappa_f, is the one that bites.)

Sensitivity, on the two-tile and the seven-tile set of the sweep, at the first and the third predicted step (mu_k = 0.33 mu_{k-1}).  The step is
formed as the chain forms it -- S = U - sum_f Y_f W_f^T (lower triangle), rhs = g_s - sum_f W_f h_f, d_f = Vinv_f (g_f - W_f^T d_s) -- from
speculative output that is wrong in one way; the single-frame mutations take the frame with the median share |W_f V_f^-1 W_f^T|_F.  The bar
resolves 3.3e-10 .. 3.5e-9 of that frame's share of A d_s (printed per case).  Every mutation fails the certificate as it is, none had to be
scaled; the smallest measured |r| / bar over the four (set, step) pairs:
    all inverses and h_f at mu_{k-1}            3.0e9        one frame's inverse at mu_{k-1}                  5.8e8
    one frame stale (V^-1, h_f, Y of z_{k-1})   9.6e8        one frame's h_f exchanged with its neighbour's   2.3e7
    one frame's Y rows one entity slot off      4.7e8        U, g_s of z_{k-1} (missed pass B rebuild)        1.3e11
"""
import numpy as np
import pytest

import direct_cases as dc
import direct_run_certificate as drc
import oracle_lib as ol
from direct_certificate import DirectCertificateError, build_system, certify_direct, entity_blocks, residual_bars
from pair_priors_restated import pair_terms
from reduced_system import prior_terms

FAMILY = {"passa_cut": "pass A", "avg_le_14": "pass A", "avg_15_30": "pass A", "avg_31_96": "pass A", "avg_gt_96": "pass A", "wide_84": "pass A",
          "worklist_F60": "pass A", "huber": "features", "intrinsics": "features", "priors": "features", "fixed": "features",
          "cams_off": "features", "markers_off": "features", "frames_off": "features", "far_start": "far start"}
WORST = {}
_RUNS = {}


class HostRun:
    """one LM run on the oracle's normal equations: zs, trace, and the system of every step"""

    def __init__(self, name, max_iters=10):
        if name == "sweep7":
            ds, x0, kw, tau, need, huber = dc.sweep_ds(7), None, {}, 1.0, 3, None
            x0 = np.asarray(ds.x_full, dtype=np.float64)
        else:
            ds, x0, kw, tau, need, huber = dc.spec_run(name)
        self.ds, self.x0, self.need, self.tau = ds, x0, need, tau
        self.opt, self.intr = kw.get("optimize", (True, True, True)), kw.get("intrinsics", False)
        self.fixed = {k: kw[k] for k in ("fixed_cams", "fixed_markers") if k in kw}
        self.priors, self.pairs = kw.get("priors"), kw.get("pair_priors")
        self.o = ol.Oracle(ds, optimize=self.opt, with_huber=kw.get("with_huber", False), huber_delta=huber or 10.0, intrinsics=self.intr)
        self.blocks = entity_blocks(ds, self.opt, self.intr)
        self._lm(max_iters)

    def merge(self, z):
        return self.o.merge_z(self.x0, z)

    def prior_blocks(self, x):
        """(Hp, Bp, cost) of the pose priors and the pair priors at x"""
        P = self.o.num_vars
        Hp, Bp, cost = np.zeros((P, P)), np.zeros(P), 0.0
        if self.priors:
            h, b, c = prior_terms(self.ds, x, self.priors, P)
            Hp, Bp, cost = Hp + h, Bp + b, cost + c
        if self.pairs:
            h, b, c, _ = pair_terms(self.ds, x, self.pairs, P)
            Hp, Bp, cost = Hp + h, Bp + b, cost + c
        return Hp, Bp, cost

    def system(self, z, mu):
        x = self.merge(z)
        H, B = self.o.normal_equations(x, res_mode=ol.RES_F32)
        Hp, Bp, _ = self.prior_blocks(x)
        return build_system(self.ds, H, B, mu, self.opt, self.intr, Hp=Hp, Bp=Bp, **self.fixed)

    def err(self, z):
        return float(np.sum(self.o.residuals(self.x0, z=z, res_mode=ol.RES_F32) ** 2)) + self.prior_blocks(self.merge(z))[2]

    def _lm(self, max_iters):
        """aar_lm_init / aar_lm_step / the loop of aar_lm_solve, restated"""
        z = self.o.extract_z(self.x0)
        prev = cur = self.err(z)
        rows = 8.0 * self.ds.num_obs
        mu, v = None, 2.0
        self.zs, self.trace, self.mus, self.steps = [z], [], [], []
        for _ in range(max_iters):
            tries, accepted, gain = 0, False, 0.0
            while tries < 6 and not accepted:
                if mu is None:
                    rs = self.system(z, 0.0)
                    self.mu0 = mu = self.tau * max(float(np.diag(rs.U)[~rs.held_e].max()), float(max(np.diag(V).max() for V in rs.V)) if rs.F else 0.0)
                rs = self.system(z, mu)
                d_s = rs.solve_s()
                d = rs.assemble(d_s, rs.backsub(d_s))
                g = rs.assemble(rs.gs, rs.gf)
                e = self.err(z + d)
                gain = (e - prev) / (0.5 * (mu * (d @ d) - d @ g))
                tries += 1
                if gain > 0 and e - prev < 0:
                    self.mus.append(mu)
                    self.steps.append(d)
                    mu, v, z, cur, accepted = mu * max(0.33, 1.0 - (2 * gain - 1) ** 3), 2.0, z + d, e, True
                else:
                    mu, v = mu * v, v * 5
            if not accepted:
                self.mus.append(None)
                self.steps.append(None)
            self.trace.append(dict(err=cur, mu=mu, gain=gain, accepted=int(accepted), tries=tries))
            self.zs.append(z)
            stop = abs(prev - cur) / rows <= 1e-4 or not accepted or cur < 1e-5
            prev = cur
            if stop:
                break
        self.classes = drc.classify(self.trace)


def _run(name):
    if name not in _RUNS:
        _RUNS[name] = HostRun(name)
    return _RUNS[name]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nfloat64 steps of the runs, per family: worst |r| / bar, worst frame ratio of the step itself | of the step read back as z1 - z0")
    for fam, w in sorted(WORST.items()):
        print("  %-12s %.3e  %.3e | %.3e  %.3e" % (fam, *w))


def _family(name):
    return FAMILY.get(name, "MFMA lists" if name.startswith(("mfma", "dense")) else "tile sweep")


@pytest.mark.parametrize("name", list(dc.SPEC_RUNS) + ["sweep7"])
def test_every_run_offers_its_predicted_steps_and_float64_stays_within_an_eighth_of_the_bar(name):
    r = _run(name)
    ks, cls = drc.pick_steps(r.trace, kinds=("predicted", "taken back", "rebuilt") if name == "far_start" else ("predicted",))
    print(name, " ".join("%s %.2f/%d" % (c, t["gain"], t["tries"]) for c, t in zip(cls, r.trace)))
    assert len(r.trace) <= 10 and cls.count("predicted") >= r.need, (name, cls)
    # (the restated rule agrees with the helper's reading of a trace: dampings, and the bit-for-bit product before a predicted step)
    for k, t in enumerate(r.trace):
        if t["accepted"]:
            assert drc.mu_used(r.trace, k, r.mu0) == r.mus[k], (name, k)
    drc.check_predicted_dampings(r.trace, r.mu0)
    if name == "far_start":
        # the run of the repairs test and of the ranks' taken-back case: a rejected try, an accepted step with gain < 0.94 followed by a
        # one-try step, and a predicted step behind a repair
        assert "rebuilt" in cls and "taken back" in cls, cls
        assert any(c == "taken back" and r.trace[k - 1]["accepted"] and r.trace[k - 1]["gain"] < 0.94 for k, c in enumerate(cls)), cls
        assert any(c == "predicted" and cls[k - 1] in ("rebuilt", "taken back") for k, c in enumerate(cls)), cls
    # the steps as a run hands them over -- zs[k + 1] - zs[k], rounded through z like the device's -- pass the certificate ...
    res = drc.certify_steps(r.ds, r.zs, r.trace, r.mu0, lambda x: r.o.normal_equations(x, res_mode=ol.RES_F32), r.merge, ks, what=name,
                            optimize=r.opt, intrinsics=r.intr, fixed=r.fixed, Hp_Bp=lambda x: r.prior_blocks(x)[:2])
    assert sum(c == "predicted" for _, c, _ in res) >= r.need
    w = WORST.setdefault(_family(name), [0.0, 0.0, 0.0, 0.0])
    for k, c, out in res:
        w[2], w[3] = max(w[2], out["ratio"]), max(w[3], out["frame_ratio"])
        # ... and the float64 step itself (the reference of tests/test_direct_certificate_host.py: d, not a difference of two pose vectors)
        # stays within an eighth of the bar
        # (its frame part once more without the restatement's inverses: np.linalg.solve on V_f, last frame first)
        rs = r.system(r.zs[k], r.mus[k])
        d_s = rs.split(r.steps[k])[0]
        d_f = np.array([np.linalg.solve(rs.V[f], rs.gf[f] - rs.W64[::-1, f, :].T @ d_s[::-1]) for f in range(rs.F - 1, -1, -1)][::-1]).reshape(rs.F, 6)
        out = certify_direct(rs, rs.assemble(d_s, d_f), r.zs[k + 1], r.blocks, "%s step %d" % (name, k))
        assert out["ratio"] <= 0.125 and out["frame_ratio"] <= 0.125, (name, k, c, out)
        w[0], w[1] = max(w[0], out["ratio"]), max(w[1], out["frame_ratio"])


def test_the_launch_counts_a_classification_implies():
    t = lambda acc, tries, gain: dict(accepted=acc, tries=tries, gain=gain, mu=1.0, err=1.0)
    trace = [t(1, 1, 2.0), t(1, 1, 0.5), t(1, 1, 2.0), t(1, 3, 2.0), t(1, 1, 2.0), t(0, 6, -1.0)]
    assert drc.classify(trace) == ["first", "predicted", "taken back", "rebuilt", "predicted", None]
    # first: k_frame_inv + 2 complements; predicted: 0 + 1; taken back: 1 + 3; rebuilt behind a predicted first try: 2 + 1 + 4;
    # predicted: 0 + 1; a rejected step whose first try was predicted: 5 + 1 + 10
    assert drc.expected_launches(trace) == (1 + 0 + 1 + 2 + 0 + 5, 2 + 1 + 3 + 5 + 1 + 11)


# ---- sensitivity: the step the chain would produce from a wrong speculation ----
def _chain_step(rs, Vinv=None, hf=None, Y=None, U=None, gs=None):
    """S = U - sum_f Y_f W_f^T (lower triangle, as the factorisation reads it), rhs = g_s - sum_f W_f h_f, d_f = Vinv_f (g_f - W_f^T d_s)"""
    n, F = len(rs.ent), rs.F
    W = rs.W64
    Vinv = rs.Vinv if Vinv is None else Vinv
    hf = np.einsum("fij,fj->fi", Vinv, rs.gf) if hf is None else hf
    Y = np.einsum("efi,fij->efj", W, Vinv) if Y is None else Y
    A = (rs.U if U is None else U) - Y.reshape(n, 6 * F) @ W.reshape(n, 6 * F).T
    A = np.tril(A) + np.tril(A, -1).T
    b = (rs.gs if gs is None else gs) - np.einsum("efj,fj->e", W, hf)
    d_s = np.linalg.solve(A, b)
    d_f = np.einsum("fij,fj->fi", Vinv, rs.gf - np.einsum("efj,e->fj", W, d_s))
    return rs.assemble(d_s, d_f)


def _median_frame(rs):
    share = np.linalg.norm(np.einsum("efi,fij,gfj->feg", rs.W64, rs.Vinv, rs.W64), axis=(1, 2))
    return int(np.argsort(share)[rs.F // 2])


MUTATIONS = ["all_at_old_mu", "one_at_old_mu", "one_stale", "hf_exchanged", "y_one_slot_off", "shared_part_stale"]
_MUT = {}


def _mutation_setup(tiles, nth):
    if (tiles, nth) not in _MUT:
        r = _run("sweep%d" % tiles)
        k = [k for k, c in enumerate(r.classes) if c == "predicted"][nth]
        mu_prev, mu_k = r.mus[k - 1], r.mus[k]
        assert mu_k == 0.33 * mu_prev
        _MUT[(tiles, nth)] = (r, k, r.system(r.zs[k], mu_k), r.system(r.zs[k], mu_prev), r.system(r.zs[k - 1], mu_k))
    return _MUT[(tiles, nth)]


@pytest.mark.parametrize("nth", [0, 2])
@pytest.mark.parametrize("tiles", [2, 7])
@pytest.mark.parametrize("kind", MUTATIONS)
def test_a_step_from_a_wrong_speculation_fails(kind, tiles, nth):
    r, k, rs, rs_mu, rs_old = _mutation_setup(tiles, nth)
    f = _median_frame(rs)
    Vinv, hf = rs.Vinv.copy(), np.einsum("fij,fj->fi", rs.Vinv, rs.gf)
    Y = np.einsum("efi,fij->efj", rs.W64, rs.Vinv)
    if kind == "all_at_old_mu":
        d = _chain_step(rs, Vinv=rs_mu.Vinv)
    elif kind == "one_at_old_mu":
        Vinv[f] = rs_mu.Vinv[f]
        d = _chain_step(rs, Vinv=Vinv)
    elif kind == "one_stale":
        Vinv[f] = rs_old.Vinv[f]
        hf[f] = rs_old.Vinv[f] @ rs_old.gf[f]
        Y[:, f, :] = rs_old.W64[:, f, :] @ rs_old.Vinv[f]
        d = _chain_step(rs, Vinv=Vinv, hf=hf, Y=Y)
    elif kind == "hf_exchanged":
        g = (f + 1) % rs.F
        hf[[f, g]] = hf[[g, f]]
        d = _chain_step(rs, hf=hf)
    elif kind == "y_one_slot_off":
        Y[:, f, :] = np.roll(Y[:, f, :], 6, axis=0)
        d = _chain_step(rs, Y=Y)
    else:
        d = _chain_step(rs, U=rs_old.U, gs=rs_old.gs)
    z0 = r.zs[k]
    # what the bar resolves in this frame: the bar of (a) against the frame's share of A d_s
    d_s = rs.split(rs.exact_step())[0]
    _, bar, _, _ = residual_bars(rs, d_s, rs.split(z0)[0], r.blocks)
    share = np.linalg.norm(rs.W64[:, f, :] @ rs.Vinv[f] @ rs.W64[:, f, :].T @ d_s)
    with pytest.raises(DirectCertificateError) as ei:
        certify_direct(rs, d, z0 + d, r.blocks, "%s, %d tiles, step %d" % (kind, tiles, k))
    print("%s, %d tiles, LM step %d (frame %d, the bar resolves %.2e of its share): %s" % (kind, tiles, k, f, bar / share, str(ei.value)[:160]))
    # the exact chain step of the same arrays passes: the failure is the mutation's
    d = _chain_step(rs)
    out = certify_direct(rs, d, z0 + d, r.blocks, "unmutated")
    assert out["ratio"] <= 0.125 and out["frame_ratio"] <= 0.125
