"""Certificate of the steps INSIDE an LM run of the direct chain -- TEST INFRASTRUCTURE ONLY, numpy only.

tests/direct_certificate.py certifies one damped step against the float64 restatement of the reduced system of the device's own normal
equations.  This module applies it, unchanged (certify_direct, build_system, entity_blocks: no new bar), to the steps an LM run takes by
itself, which is the only place where the speculative path of damped_try (csrc/ba_capi.hip) runs: the trial point's pass A inverts
V_f + 0.33 mu I ahead of time (passA_epilogue and its wrench twin, csrc/eval_kernels.hip: Vinv, h_f, with the MFMA kernel the panels
Wd / Yd), the trial's Schur complement is subtracted before the host has decided, behind a communicator S | rhs | g0 is all-reduced with
the step's scalars, and with AAR_SPEC_CHOL the factorisation is queued as well.  When the step is accepted with gain >= 0.94 the next try
runs none of k_frame_inv, k_schur_fill, k_schur: it factorises what is there.

    run            lm_solve with a step callback that records z after every step: (zs, trace)
    damping        mu_used(trace, k, mu0): the trace records the damping AFTER step k; the accepted try of step k used the damping after
                   step k - 1 (mu0 = tau max diag H of the device's own H at the start), times 2, 10, 50, ... per rejected try
    classes        every accepted step k: "first" (k = 0), "rebuilt" (tries > 1, or the step before was not accepted: the blocks of the
                   current point were rebuilt from the observations), "predicted" (tries = 1, step k - 1 accepted with
                   max(0.33, 1 - (2 gain - 1)^3) == 0.33: nothing is launched for the system), "taken back" (tries = 1, step k - 1 accepted
                   with a larger factor: the speculative complement is taken back, k_frame_inv, a fresh complement)
                   on a predicted step trace[k - 1]["mu"] == 0.33 mu_used(k - 1) bit for bit (aar_lm_step forms it with that expression)
    evaluation     AFTER the run, never between steps: an evaluation clears blocks_valid and forces rebuild_current, the path this
                   certificate is not about.  H, B = eval_normal_equations(merge_z(x0, zs[k])), the system at mu_k, certify_direct on
                   zs[k + 1] - zs[k]
    which steps    the FIRST predicted steps of the run (six), none skipped.  Early steps are the ones worth certifying: near convergence
                   the step is small against ulp |z|, the certificate's slack term (the rounding of z0 + d) then is most of the bar and
                   hides everything -- hence the first six and not a spread over the run.  Every caller states how many predicted steps it
                   must have certified; a run that did not offer them fails (the premise, not a result).
    launches       one GPU, kernel profiling on (it keeps the first step's head start out of aar_lm_init and changes nothing else on one
                   GPU): expected_launches(trace) gives the k_frame_inv and launch_schur counts the classification implies
"""
import numpy as np

from direct_certificate import build_system, certify_direct, entity_blocks

N_PREDICTED = 6            # the first predicted steps of a run that are certified


def mu_used(trace, k, mu0):
    """damping of the ACCEPTED try of step k: the trace records the damping AFTER the step (aar_lm_step: out->mu = pb->mu), the rejected tries
    before it multiplied it by v = 2, 10, 50, ..."""
    mu = mu0 if k == 0 else trace[k - 1]["mu"]
    v = 2.0
    for _ in range(trace[k]["tries"] - 1):
        mu = mu * v
        v = v * 5
    return mu


def factor(gain):
    """what an accepted step multiplies its damping with (aar_lm_step; libs/sparselevmarq.h:410 of the reference)"""
    return max(0.33, 1.0 - (2.0 * gain - 1.0) ** 3)


def classify(trace):
    """per step: None (not accepted) | "first" | "predicted" | "taken back" | "rebuilt" """
    out = []
    for k, t in enumerate(trace):
        if not t["accepted"]:
            out.append(None)
        elif t["tries"] > 1 or (k > 0 and not trace[k - 1]["accepted"]):
            out.append("rebuilt")
        elif k == 0:
            out.append("first")
        else:
            out.append("predicted" if factor(trace[k - 1]["gain"]) == 0.33 else "taken back")
    return out


def first_try_predicted(trace, k):
    """is the FIRST try of step k (accepted or not, whatever follows it) one that finds its system ready?"""
    return k > 0 and bool(trace[k - 1]["accepted"]) and factor(trace[k - 1]["gain"]) == 0.33


def expected_launches(trace):
    """(k_frame_inv launches, launch_schur calls) of a run on one GPU with kernel profiling on.  Per try: a predicted first try launches no
    k_frame_inv and one Schur complement (the next trial's, speculative); every other try launches k_frame_inv and two complements (its own,
    the next trial's); a first try after an accepted step with another factor than 0.33 takes the speculative complement back first (a third)."""
    finv = schur = 0
    for k, t in enumerate(trace):
        tries = max(int(t["tries"]), 1)
        if first_try_predicted(trace, k):
            finv += tries - 1
            schur += 1 + 2 * (tries - 1)
        else:
            finv += tries
            schur += 2 * tries + (1 if k > 0 and trace[k - 1]["accepted"] else 0)
    return finv, schur


def check_predicted_dampings(trace, mu0):
    """trace[k - 1]["mu"] == 0.33 mu_used(k - 1) bit for bit before every predicted step.  (k - 1 = 0: mu_used is mu0, which the caller
    takes from an evaluation of its own -- a second summation of the same diagonal, in another order where the blocks are summed with
    atomics --, so there the two may differ by the rounding of that sum: four ulp are allowed, and only there.)"""
    for k, c in enumerate(classify(trace)):
        if c == "predicted":
            want = 0.33 * mu_used(trace, k - 1, mu0)
            got = trace[k - 1]["mu"]
            if k - 1 == 0:
                assert abs(got - want) <= 4 * np.spacing(want), (k, got, want)
            else:
                assert got == want, (k, got, want)


def record_run(p, x0, params):
    """(zs, trace, report): z at the start and after every step of p.lm_solve(x0, params)"""
    zs = [p.extract_z(x0)]
    p.set_step_callback(lambda z: zs.append(z))
    try:
        _, rep = p.lm_solve(x0, params=params)
    finally:
        p.set_step_callback(None)
    return zs, rep["trace"], rep


def pick_steps(trace, kinds=("predicted",), n_predicted=N_PREDICTED, n_other=3):
    """the steps to certify: the first n_predicted predicted steps, the first n_other of every other kind asked for"""
    cls = classify(trace)
    ks = []
    for kind in kinds:
        ks += [k for k, c in enumerate(cls) if c == kind][:n_predicted if kind == "predicted" else n_other]
    return sorted(ks), cls


def certify_steps(ds, zs, trace, mu0, normal_equations, merge_z, ks, what="", optimize=(True, True, True), intrinsics=False, fixed=None,
                  Hp_Bp=None, frame_rows=None):
    """certify steps ks of a recorded run.  normal_equations(x) -> (H, B) at the full vector x (the device's own, evaluated AFTER the run;
    on the host the oracle's); merge_z(z) -> x; Hp_Bp(x) -> the priors' blocks where H does not carry them (the oracle's).
    Returns [(k, class, certify_direct's dict)]."""
    blocks = entity_blocks(ds, optimize, intrinsics)
    cls = classify(trace)
    out = []
    for k in ks:
        assert trace[k]["accepted"] and k + 1 < len(zs), (k, len(zs))
        mu = mu_used(trace, k, mu0)
        x = merge_z(zs[k])
        H, B = normal_equations(x)[:2]
        Hp, Bp = Hp_Bp(x) if Hp_Bp is not None else (None, None)
        rs = build_system(ds, H, B, mu, optimize, intrinsics, Hp=Hp, Bp=Bp, **(fixed or {}))
        res = certify_direct(rs, zs[k + 1] - zs[k], zs[k + 1], blocks, "%s: LM step %d, %s (mu %.6g, %d tries, gain before %.4g)"
                             % (what, k, cls[k], mu, trace[k]["tries"], trace[k - 1]["gain"] if k else 0.0))
        out.append((k, cls[k], res))
    return out
