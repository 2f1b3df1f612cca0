"""The rotation-log terms on the device -- so3_log and so3_jr_inv of csrc/so3.hpp at every call site: k_prior, k_pair_prior, pair_terms<true>
through aar_track_smooth_system, the live tracker's pair terms -- near zero, at every series switch and up to a half turn, against the mp
reference tests/rotation_reference.py (residuals from their definitions, Jacobians by differences at 60 digits; pinned on the CPU by
tests/test_rotation_reference_host.py).  Needs a real MI355X.

Cases (tests/rotation_edge_cases.py): 16 residual angles + "nearest to pi" x 12 axes x the classes of the poses' own rotation vectors.

Bars: rotation_edge_cases.F64_WORST holds what a careful float64 evaluation of the same quantities loses against mp on the CPU, per site and
quantity; the device is held to 8 x that (rotation_edge_cases.bar), plus what the test's own arithmetic costs:

  k_prior, k_pair_prior   The priors' share of H and B is eval_normal_equations of the problem minus that of its prior-less twin, both
                          deterministic.  The information matrices are scaled by a power of two s >= 2^40 max diag(H_twin), so the data's entries
                          are below 1e-12 of the priors' and the difference costs two roundings of the sum itself: + 2.3e-16 on the scaled H and B.
  smooth system           The pair share is system(sigma_1) - system(sigma_2), sigma_2 = 2^10 sigma_1, lambda_1 = 1 / sigma_1^2 = a power of two
                          >= 2^40 max diag(data), lambda_2 = 2^-20 lambda_1 (still 2^20 x the data): the data blocks cancel, the pair blocks are
                          linear in lambda, and the difference is the pair share at lambda_1 - lambda_2.  It amplifies the kernel's own error by
                          (lambda_1 + lambda_2) / (lambda_1 - lambda_2) = 1 + 2^-19 and adds three roundings: the bar is 8 x F64 x (1 + 2^-19) + 3.4e-16,
                          i.e. the difference costs no digit.  The prior cost needs no difference: it is reported apart from the data cost.
  summed costs            a sum of n non-negative terms in any order carries at most (n - 1) 2^-53 relative: added to the cost bar.

Strided loops: k_prior with 258 priors and k_pair_prior with 507 pairs (the second round of `p += 256` and of the lane-strided cost sums), at
generic angles, against reduced_system.prior_terms / pair_priors_restated.pair_terms at those modules' bars (e 1e-12, cost 1e-12 relative,
blocks test_gpu_pair_priors.BLOCK_BAR with the information at 1e-3 of the data's diagonal).  No earlier test has n_prior or n_pair above 256.

The smooth system cannot see an error of so3_jr_inv's k near pi, and that is a property of the term, not of the test: with an isotropic rotation
information lambda I the pair's blocks are lambda M^T M, and d(J^T J) for dJ = -dk th^2 P (P = I - n n^T) is -2 dk th^2 (1 - k th^2) P, where
1 - k th^2 = (th/2) cot(th/2) vanishes at pi; B = -lambda J^T phi does not see k at all (phi is an eigenvector).  The priors carry full 6 x 6
information matrices and do see it.  The live tracker's check is at cost level only (|phi| = theta whatever the axis); its Jacobians are the
smooth system's.

MEASURED on an MI355X, worst over the list ("plain" / "2pi" classes; H and B scaled, e absolute, summed cost relative):

  with so3_jr_inv's k = 1/th^2 - (1 + cos th) / (2 th sin th)  (the commit before this file)
    k_prior        pi - 1e-6:  H 4.7e-11  B 2.9e-11     pi - 1e-9:  H 5.9e-10  B 3.0e-10     pi - 1e-12:  H 6.8e-13  B 2.3e-13     (bars 2.2e-14, 1.3e-13: FAIL)
    k_pair_prior   pi - 1e-6:  H 6.0e-11  B 3.2e-11     pi - 1e-9:  H 6.3e-10  B 2.9e-10     pi - 1e-12:  H 4.5e-13  B 2.9e-13     (bars 3.1e-14, 1.8e-13: FAIL)
    every other angle, every e and cost, the smooth system, the live tracker and the strided problems: inside their bars, as below

  with k = 1/th^2 - cot(th/2) / (2 th), cot(th/2) = (1 + cos th) / sin th below pi / 2 and sin th / (1 - cos th) above  (this commit; the half-angle
  form cos(th/2) / sin(th/2) measured the same to two digits, but its second sincos made one instance of the live kernels round differently from
  another, which tests/test_gpu_live_motion.py forbids bit for bit)
    k_prior        e 6.7e-15 / 2.4e-15 (generic side of the near-pi switch; elsewhere <= 1.8e-15)   H 7.3e-15 / 3.4e-13 (2pi: theta = 0.01 + 1e-6)
                   B 3.0e-14 / 3.4e-14   cost 5.8e-16          at pi - 1e-6 .. pi - 1e-12: H <= 7.3e-15, B <= 4.2e-15; nearest pi: H 3.8e-16, e 4.4e-16
    k_pair_prior   e 6.5e-15 / 4.4e-15   H 8.6e-15 / 3.2e-13   B 2.3e-14 / 1.2e-13   cost 9.6e-16      at pi - 1e-6 .. pi - 1e-12: H <= 8.6e-15 (2pi 3.2e-14)
    smooth system  H 7.7e-16   B 1.3e-15   prior cost 1.2e-16 (with rel_motion), 1.1e-16 (without); near pi H <= 5.4e-16
    live tracker   |initial_cost - reference| <= 3.9e-3 of 1e13 (4e-16 relative; bars 6e-2 .. 8e-2) in all ten pushes: lag 1 and 3, fixed and
                   marginal anchor, a bank of two with the motion model
    strided loops  258 priors: e 6.1e-16, cost 1.3e-16, blocks 4.8e-14; 507 pairs: e 7.8e-16, cost 8.8e-16, blocks 3.6e-15 (bar 1.7e-12)
  Wall time of the file: 20 s, of which the mp reference of the 1740 + 1548 + 2 x 195 cases takes 12 s.
"""
import math

import numpy as np
import pytest

import aar
import rotation_edge_cases as ec
import rotation_reference as rr
from aar import Problem
from reduced_system import slot_col

pytestmark = pytest.mark.gpu

TWIN_ROUNDINGS = 2 * 2.0 ** -53 * 1.01
SMOOTH_AMPLIFY, SMOOTH_ROUNDINGS = 1.0 + 2.0 ** -19, 3 * 2.0 ** -53 * 1.01


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def free_slots(ds):
    return [("camera", c) for c in range(ds.num_cams) if c != ds.root_cam], [("marker", m) for m in range(ds.num_markers) if m != ds.root_marker]


def pow2_above(v):
    return 2.0 ** math.ceil(math.log2(v))


def angle_tag(case):
    if "nearest" in case.name:
        return "nearest pi"
    return "%.17g" % case.theta


class Worst:
    """worst distance / bar per (residual angle, quantity), and the cases over the bar"""

    def __init__(self, site):
        self.site, self.by_angle, self.over = site, {}, []

    def add(self, case, quantity, value, bar):
        assert np.isfinite(value), (case, quantity, value)
        key = (angle_tag(case), quantity + ("" if ec.group(case) == "plain" else " [2pi]"))
        if value > self.by_angle.get(key, (-1.0, 0.0))[0]:
            self.by_angle[key] = (value, bar)
        if not value <= bar:
            self.over.append((case.name, quantity, value, bar))

    def report(self):
        angles = []
        for a, _ in self.by_angle:
            if a not in angles:
                angles.append(a)
        for a in angles:
            print("%s theta %-22s %s" % (self.site, a, "  ".join("%s %.2e (bar %.1e)" % (q, v, b) for (aa, q), (v, b) in sorted(self.by_angle.items()) if aa == a)))

    def check(self):
        self.report()
        assert not self.over, "%d over the bar, first: %r" % (len(self.over), self.over[:8])


# ---------------------------------------------------------------- k_prior
def test_prior_terms_at_every_edge():
    ds = aar.synth(2, num_markers=60, num_frames=3)
    fc, fm = free_slots(ds)
    slots = fc + fm
    cases, ref = ec.prior_cases(), ec.prior_reference()
    w = Worst("k_prior")
    for c0 in range(0, len(cases), len(slots)):
        chunk = cases[c0:c0 + len(slots)]
        x = np.array(ds.x_full, dtype=np.float64)
        for (kind, i), c in zip(slots, chunk):
            col = slot_col(ds, kind, i)
            x[col:col + 6] = c.poses[0]
        with Problem(ds, solver="direct", deterministic=True) as tw:
            Ht, Bt, _ = tw.eval_normal_equations(x)
        s = pow2_above(2.0 ** 40 * float(np.diag(Ht).max()))
        priors = [(kind, i, c.poses[1], s * c.info) for (kind, i), c in zip(slots, chunk)]
        with Problem(ds, solver="direct", deterministic=True, priors=priors) as p:
            Hc, Bc, _ = p.eval_normal_equations(x)
            e, cost = p.eval_priors(x)
        dH, dB = Hc - Ht, Bc - Bt
        cref = 0.0
        for n, ((kind, i), c) in enumerate(zip(slots, chunk)):
            col = slot_col(ds, kind, i)
            r = ref[c.name]
            de, dh, db, _ = rr.distances(e[n], dH[col:col + 6, col:col + 6] / s, dB[col:col + 6] / s, r.cost, r)
            w.add(c, "e", de, ec.bar("prior", c, "e"))
            w.add(c, "H", dh, ec.bar("prior", c, "H") + TWIN_ROUNDINGS)
            w.add(c, "B", db, ec.bar("prior", c, "B") + TWIN_ROUNDINGS)
            cref += r.cost
        cbar = max(ec.bar("prior", c, "cost") for c in chunk) + (len(chunk) - 1) * 2.0 ** -53
        w.add(chunk[0], "cost(sum)", abs(cost / s - cref) / cref, cbar)
    w.check()


# ---------------------------------------------------------------- k_pair_prior
def pair_runs():
    """(case, way): every case both ends free with a < b or a > b (alternating); every near-pi case all three ways"""
    out = []
    for n, c in enumerate(ec.pair_cases()):
        if ec.is_near_pi(c):
            out += [(c, "a<b"), (c, "a>b"), (c, "fixed_a" if n % 2 else "fixed_b")]
        else:
            out.append((c, "a<b" if n % 2 else "a>b"))
    return out


def test_pair_prior_terms_at_every_edge():
    ds = aar.synth(2, num_markers=60, num_frames=3)
    fc, fm = free_slots(ds)
    seats = [(fc[0], fc[1])] + [(fm[k], fm[k + 1]) for k in range(0, len(fm) - 1, 2)]      # disjoint (lower, higher) pairs of one kind
    runs, ref = pair_runs(), ec.pair_reference()
    w = Worst("k_pair_prior")
    ways = set()
    for c0 in range(0, len(runs), len(seats)):
        chunk = runs[c0:c0 + len(seats)]
        x = np.array(ds.x_full, dtype=np.float64)
        placed, fixed_c, fixed_m = [], [], []
        for ((kind, lo), (_, hi)), (c, way) in zip(seats, chunk):
            a, b = (hi, lo) if way == "a>b" else (lo, hi)
            x[slot_col(ds, kind, a):slot_col(ds, kind, a) + 6] = c.poses[0]
            x[slot_col(ds, kind, b):slot_col(ds, kind, b) + 6] = c.poses[1]
            held = {"fixed_a": a, "fixed_b": b}.get(way)
            if held is not None:
                (fixed_c if kind == "camera" else fixed_m).append(held)
            placed.append((kind, a, b, held, c))
            ways.add(way)
        kw = dict(solver="direct", deterministic=True, fixed_cams=fixed_c or None, fixed_markers=fixed_m or None)
        with Problem(ds, **kw) as tw:
            Ht, Bt, _ = tw.eval_normal_equations(x)
        s = pow2_above(2.0 ** 40 * float(np.diag(Ht).max()))
        pairs = [(kind, a, b, c.poses[2], s * c.info) for kind, a, b, _, c in placed]
        with Problem(ds, pair_priors=pairs, **kw) as p:
            Hc, Bc, _ = p.eval_normal_equations(x)
            e, cost = p.eval_pair_priors(x)
        dH, dB = Hc - Ht, Bc - Bt
        cref = 0.0
        for n, (kind, a, b, held, c) in enumerate(placed):
            r = ref[c.name]
            ca, cb = slot_col(ds, kind, a), slot_col(ds, kind, b)
            idx = np.r_[ca:ca + 6, cb:cb + 6]
            got_H, got_B = dH[np.ix_(idx, idx)] / s, dB[idx] / s
            if held is not None:
                # a fixed end is a constant of its term: its rows, its columns and the cross block stay the twin's, bit for bit
                ch = slot_col(ds, kind, held)
                assert np.array_equal(Hc[ch:ch + 6], Ht[ch:ch + 6]) and np.array_equal(Hc[:, ch:ch + 6], Ht[:, ch:ch + 6]) and np.array_equal(Bc[ch:ch + 6], Bt[ch:ch + 6])
                keep = np.r_[6:12] if held == a else np.r_[0:6]
                sub = type("Sub", (), dict(e=r.e, H=r.H[np.ix_(keep, keep)], B=r.B[keep], cost=r.cost))
                de, dh, db, _ = rr.distances(e[n], got_H[np.ix_(keep, keep)], got_B[keep], r.cost, sub)
            else:
                de, dh, db, _ = rr.distances(e[n], got_H, got_B, r.cost, r)      # both diagonal blocks, the cross block both ways, B of both ends
            w.add(c, "e", de, ec.bar("pair", c, "e"))
            w.add(c, "H", dh, ec.bar("pair", c, "H") + TWIN_ROUNDINGS)
            w.add(c, "B", db, ec.bar("pair", c, "B") + TWIN_ROUNDINGS)
            cref += r.cost
        cbar = max(ec.bar("pair", c, "cost") for _, _, _, _, c in placed) + (len(placed) - 1) * 2.0 ** -53
        w.add(placed[0][4], "cost(sum)", abs(cost / s - cref) / cref, cbar)
    assert ways == {"a<b", "a>b", "fixed_a", "fixed_b"}
    w.check()


# ---------------------------------------------------------------- pair_terms<true> through the smoothed tracker's system
def test_smooth_system_pair_terms_at_every_edge():
    F = ec.BETWEEN_FRAMES
    ds = aar.synth(2, num_frames=F)
    z, rel, has, cases = ec.between_track(ec.synthetic_track(F))
    n0 = 6 * (ds.num_cams - 1) + 6 * (ds.num_markers - 1)
    x = np.array(ds.x_truth, dtype=np.float64)
    x[n0:n0 + 6 * F] = z.reshape(-1)
    w = Worst("smooth system")
    with Problem(ds) as p:
        gd0 = p.track_smooth_system(x, 0.05, 0.02, 1.0)[0]
        lam1 = pow2_above(2.0 ** 40 * float(np.einsum("fii->fi", gd0).max()))
        if math.log2(lam1) % 2:
            lam1 *= 2.0
        s1 = 1.0 / math.sqrt(lam1)              # a power of two: 1 / (s1 s1) = lam1 exactly
        s2 = s1 * 2.0 ** 10
        assert 1.0 / (s1 * s1) == lam1 and 1.0 / (s2 * s2) == lam1 * 2.0 ** -20
        # sigma_trans = sigma_rot / 2: lambda_trans = 4 lambda_rot, so a mix-up of the two shows
        dl_r, dl_t = lam1 - lam1 * 2.0 ** -20, 4.0 * (lam1 - lam1 * 2.0 ** -20)
        for tag, rm, hh in (("rel", rel, has), ("null", None, np.zeros_like(has))):
            d1, o1, r1, _, c1 = p.track_smooth_system(x, s1, 0.5 * s1, 1.0, rel_motion=rm)
            d2, o2, r2, _, c2 = p.track_smooth_system(x, s2, 0.5 * s2, 1.0, rel_motion=rm)
            terms = ec.between_reference(cases, hh, dl_r, dl_t)
            rd, ro, rb, _ = rr.assemble_chain(terms)
            pc = np.array([t.cost for t in terms])
            eH, eB = rr.chain_distances(d1 - d2, o1 - o2, r1 - r2, rd, ro, rb, pc)
            for f, c in enumerate(cases):
                if tag == "null" and has[f]:
                    continue          # (without rel_motion the first 192 pairs are the track's own small motions: ordinary, and not the list)
                w.add(c, "H " + tag, eH[f], ec.bar("between", c, "H") * SMOOTH_AMPLIFY + SMOOTH_ROUNDINGS)
                w.add(c, "B " + tag, eB[f], ec.bar("between", c, "B") * SMOOTH_AMPLIFY + SMOOTH_ROUNDINGS)
            # the prior cost at sigma_1, reported apart from the data cost: lambda_1 / (lambda_1 - lambda_2) times the reference's
            cref = float(sum(t.cost_mp for t in terms) / rr.M.mpf(1.0 - 2.0 ** -20))
            w.add(cases[0], "cost(sum) " + tag, abs(c1[1] - cref) / cref, ec.bar("between", cases[0], "cost") + (len(cases) - 1) * 2.0 ** -53)
    w.check()


# ---------------------------------------------------------------- the strided loops
def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _spd(rng, scale):
    A = rng.standard_normal((6, 6))
    return scale * (A @ A.T + 6 * np.eye(6))


def test_more_than_256_priors_and_pairs_take_the_second_round():
    import pair_priors_restated as ppr
    import reduced_system as rs
    from test_gpu_pair_priors import BLOCK_BAR, make_pair

    ds = aar.synth(3, num_cams=4, num_markers=256, num_frames=6)
    fc, fm = free_slots(ds)
    rng = np.random.default_rng(5)
    x = np.array(ds.x_full, dtype=np.float64)
    with Problem(ds, solver="direct", deterministic=True) as tw:
        Ht, Bt, _ = tw.eval_normal_equations(x)
    P = len(Bt)
    scale = 1e-3 * float(np.diag(Ht).max()) / 12.0          # (as test_gpu_pair_priors: the condition BLOCK_BAR was measured under)
    priors = []
    for kind, i in fc + fm:
        col = slot_col(ds, kind, i)
        priors.append((kind, i, x[col:col + 6] + np.r_[0.3 * rng.standard_normal(3), 0.05 * rng.standard_normal(3)], _spd(rng, scale)))
    assert len(priors) > 256
    with Problem(ds, solver="direct", deterministic=True, priors=priors) as p:
        Hc, Bc, _ = p.eval_normal_equations(x)
        e, cost = p.eval_priors(x)
    Hp, Bp, cref = rs.prior_terms(ds, x, priors, P)
    eref = np.array([rs.prior_e(x[slot_col(ds, k, i):slot_col(ds, k, i) + 6], xp) for k, i, xp, _ in priors])
    worst = max(max(_rel((Hc - Ht)[c:c + 6, c:c + 6], Hp[c:c + 6, c:c + 6]), _rel((Bc - Bt)[c:c + 6], Bp[c:c + 6]))
                for c in (slot_col(ds, k, i) for k, i, _, _ in priors))
    print("258 priors: e %.2e, cost %.2e, blocks %.2e" % (np.abs(e - eref).max(), abs(cost - cref) / cref, worst))
    assert np.abs(e - eref).max() < 1e-12 and abs(cost - cref) <= 1e-12 * cref and worst < BLOCK_BAR
    mask = np.ones((P, P), bool)
    for k, i, _, _ in priors:
        c = slot_col(ds, k, i)
        mask[c:c + 6, c:c + 6] = False
    assert np.array_equal(Hc[mask], Ht[mask])

    ms = [m for _, m in fm]
    spec = [("marker", ms[i], ms[i + 1]) if i % 2 else ("marker", ms[i + 1], ms[i]) for i in range(len(ms) - 1)] + \
           [("marker", ms[i], ms[i + 2]) for i in range(len(ms) - 2)]
    assert len(spec) > 256
    pairs = [make_pair(ds, x, rng, k, a, b, ang=0.3 * (1 + rng.random()), info=_spd(rng, scale)) for k, a, b in spec]
    with Problem(ds, solver="direct", deterministic=True, pair_priors=pairs) as p:
        Hc, Bc, _ = p.eval_normal_equations(x)
        e, cost = p.eval_pair_priors(x)
    Hp, Bp, cref, touched = ppr.pair_terms(ds, x, pairs, P)
    eref = ppr.pair_residuals(ds, x, pairs)
    worst = 0.0
    for ci, cj in set(touched):
        blk = (slice(ci, ci + 6), slice(cj, cj + 6))
        worst = max(worst, _rel((Hc - Ht)[blk], Hp[blk]))
        if ci == cj:
            worst = max(worst, _rel((Bc - Bt)[ci:ci + 6], Bp[ci:ci + 6]))
    print("%d pairs: e %.2e, cost %.2e, blocks %.2e" % (len(pairs), np.abs(e - eref).max(), abs(cost - cref) / cref, worst))
    assert np.abs(e - eref).max() < 1e-12 and abs(cost - cref) <= 1e-12 * cref and worst < BLOCK_BAR


# ---------------------------------------------------------------- the live tracker's pair terms: a cost-level check of the wiring
LIVE_SROT, LIVE_STRANS = 2.0 ** -20, 2.0 ** -10      # stiff on purpose: the prior cost of a half turn (~1e13) must not drown in the data cost
LIVE_TURNS = [(3.1, ec.AXES[9]), (ec.PI - 1e-6, ec.AXES[10])]


def _live_inputs():
    import smooth_cases as sc
    import track_restated as tr

    n = 6 + len(LIVE_TURNS)
    ds = aar.synth(2, num_frames=n)
    x0 = sc.track_start(ds)
    return ds, tr.TrackData(ds, x0), sc.copy_of(ds, x_full=x0), n


def _frame_obs(ds, f):
    sel = np.asarray(ds.obs_frame) == f
    return ds.obs_cam[sel], ds.obs_marker[sel], ds.obs_uv[sel]


def _expected_initial_cost(td, frames, poses, times, anchor, marginal, rel_of):
    """(data, prior, marginal) cost of a window at its start: track_restated.frame_error per frame; the between factors by the mp reference
    (pair i ends at window frame i; pair 0 is the anchor pair) at L = diag(1 / (sigma_rot^2 dt) x3, 1 / (sigma_trans^2 dt) x3); the marginal
    prior (z_0 - m)^T L_m (z_0 - m) in its place when there is one"""
    import track_restated as tr

    data = sum(tr.frame_error(td.frame(f), z, -1.0) for f, z in zip(frames, poses))
    prior, marg = rr.M.mpf(0), 0.0
    for i, f in enumerate(frames):
        if i == 0 and marginal is not None:
            d = poses[0] - marginal[1]
            marg = float(d @ marginal[0] @ d)
            continue
        if i == 0 and anchor is None:
            continue
        za, ta = anchor if i == 0 else (poses[i - 1], times[i - 1])
        dt = times[i] - ta
        lam = [1.0 / (LIVE_SROT * LIVE_SROT * dt)] * 3 + [1.0 / (LIVE_STRANS * LIVE_STRANS * dt)] * 3
        rel = rel_of.get(f)
        e = rr.between_e(rr.mpv(za), rr.mpv(poses[i]), None if rel is None else rr.mpv(rel))
        prior += sum(rr.M.mpf(l) * v * v for l, v in zip(lam, e))
    return data, float(prior), marg


def _check_initial_cost(tag, g, data, prior, marg, pairs, w):
    """|initial_cost - (data + prior + marginal)| <= 1e-10 data (the bar E_f is held to against frame_error, tests/test_gpu_live_detections.py)
    + (8 x the float64 cost figure + (pairs - 1) 2^-53) prior + 1e-12 marginal (a float64 quadratic form on both sides) + 2^-52 total"""
    want = data + prior + marg
    tol = 1e-10 * data + (ec.FACTOR * ec.F64_WORST["between"]["plain"]["cost"] + max(pairs - 1, 0) * 2.0 ** -53) * prior + 1e-12 * marg + 2.0 ** -52 * want
    d = abs(g["initial_cost"] - want)
    print("%s: initial cost %.17g, data %.6g prior %.6g marginal %.6g, distance %.3e (bar %.3e)" % (tag, g["initial_cost"], data, prior, marg, d, tol))
    w.append((tag, d, tol))


@pytest.mark.parametrize("lag,anchor", [(1, "fixed"), (3, "fixed"), (1, "marginal"), (3, "marginal")])
def test_live_tracker_initial_cost_after_a_half_turn(lag, anchor):
    ds, td, sol, n = _live_inputs()
    prm = aar.lm_default_params(max_iters=3)
    times = np.arange(n, dtype=np.float64)
    checks = []
    with aar.Tracker(sol, lag=lag, smooth=True, sigma_rot=LIVE_SROT, sigma_trans=LIVE_STRANS, anchor=anchor, params=prm,
                     max_obs_per_frame=int(np.bincount(ds.obs_frame, minlength=n).max())) as t:
        win, unc = None, None
        for f in range(n):
            k = f - (n - len(LIVE_TURNS))
            if k >= 0:
                prev = win["poses"][-1]
                init = np.r_[rr.partner_vector(prev[:3], LIVE_TURNS[k][0], LIVE_TURNS[k][1], "own"), prev[3:]]
            else:
                init = td.z0[f]
            full = win is not None and win["n"] == lag + 1
            frames = ([] if win is None else list(win["frame_index"][1 if full else 0:])) + [f]
            poses = ([] if win is None else list(win["poses"][1 if full else 0:])) + [init]
            anc = None
            if full:
                anc = (win["poses"][0], times[int(win["frame_index"][0])])
            elif win is not None and win["anchor_pose"] is not None:
                anc = (win["anchor_pose"], times[int(win["frame_index"][0]) - 1])
            marg = None
            if anchor == "marginal":
                anc = None
                if unc is not None and unc["has_marginal"]:
                    assert unc["marginal_index"] == frames[0]
                    marg = (unc["marginal_info"], unc["marginal_mean"])
            g = t.push(times[f], *_frame_obs(ds, f), pose_init=init)
            data, prior, mc = _expected_initial_cost(td, frames, poses, [times[int(i)] for i in frames], anc, marg, {})
            if k >= 0:
                _check_initial_cost("lag %d %s turn %.17g" % (lag, anchor, LIVE_TURNS[k][0]), g, data, prior, mc, len(frames), checks)
                assert prior > 1e3 * data          # the half turn is what the cost consists of
            win, unc = t.window(), (t.uncertainty() if anchor == "marginal" else None)
    assert len(checks) == len(LIVE_TURNS)
    assert all(d <= tol for _, d, tol in checks), checks


def test_live_bank_with_motion_model_initial_cost_after_a_half_turn():
    ds, td, sol, n = _live_inputs()
    prm = aar.lm_default_params(max_iters=3)
    times = np.arange(n, dtype=np.float64)
    lag, B = 1, 2
    checks = []
    with aar.TrackerBank([sol, sol], lag=lag, smooth=True, sigma_rot=LIVE_SROT, sigma_trans=LIVE_STRANS, params=prm, motion="cv",
                         max_obs_per_frame=int(np.bincount(ds.obs_frame, minlength=n).max())) as bank:
        wins, rel_of = [None] * B, [{} for _ in range(B)]
        for f in range(n):
            k = f - (n - len(LIVE_TURNS))
            inits, pre = [], []
            for b in range(B):
                win = wins[b]
                if k >= 0:
                    th, ax = LIVE_TURNS[(k + b) % len(LIVE_TURNS)]          # the two members take the two turns in opposite order
                    prev = win["poses"][-1]
                    init = np.r_[rr.partner_vector(prev[:3], th, ax, "own"), prev[3:]]
                else:
                    th, init = None, td.z0[f]
                full = win is not None and win["n"] == lag + 1
                frames = ([] if win is None else list(win["frame_index"][1 if full else 0:])) + [f]
                poses = ([] if win is None else list(win["poses"][1 if full else 0:])) + [init]
                anc = None
                if full:
                    anc = (win["poses"][0], times[int(win["frame_index"][0])])
                elif win is not None and win["anchor_pose"] is not None:
                    anc = (win["anchor_pose"], times[int(win["frame_index"][0]) - 1])
                inits.append(init)
                pre.append((th, frames, poses, anc))
            gs = bank.push(times[f], [_frame_obs(ds, f)] * B, pose_init=inits)
            for b in range(B):
                m = bank.last_motion(b)
                rel_of[b][f] = np.array(m["rel"], dtype=np.float64)
                th, frames, poses, anc = pre[b]
                data, prior, _ = _expected_initial_cost(td, frames, poses, [times[int(i)] for i in frames], anc, None, rel_of[b])
                if k >= 0:
                    _check_initial_cost("bank member %d turn %.17g" % (b, th), gs[b], data, prior, 0.0, len(frames), checks)
                    assert prior > 1e3 * data
                wins[b] = bank.window(b)
        assert any(np.any(r != 0.0) for r in rel_of[0].values())          # the model did measure a motion
    assert len(checks) == B * len(LIVE_TURNS)
    assert all(d <= tol for _, d, tol in checks), checks
