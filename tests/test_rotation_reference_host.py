"""Pins of the mp reference tests/rotation_reference.py and of the case list tests/rotation_edge_cases.py, before anything leans on them.  CPU only.

1. exp(log Q) = Q to 1e-40 over every residual rotation of the list; log against scipy's Rotation.as_rotvec at generic angles.
2. The mp-differenced Jacobian of the pose prior against J_r(phi)^-1 J_l(w)^T evaluated in mp from the textbook closed forms
   (J_l = I + (1 - cos t)/t^2 K + (t - sin t)/t^3 K^2, J_r^-1 = I + K/2 + (1/t^2 - (1 + cos t)/(2 t sin t)) K^2; series below 1e-3): the numerical
   derivative IS the formula the kernels claim to implement.  Bar 1e-20: the difference quotient is good to 1e-24 (rotation_reference's
   docstring), the closed forms at 60 digits to ~1e-20 where t - sin t cancels 40 digits (t = 1e-20).  Measured: 3.5e-29.
3. The existing float64 restatements against the reference on every case below 3.0 rad (they do not claim more): measured worst distances
   (e absolute; H and B in the scaled measure, with and without the "2pi" classes of item 4)
       reduced_system.prior_e 1.3e-15, prior_J -> H 3.2e-13 / B 1.2e-13 (2pi: 5.4e-14 / 2.1e-14)
       pair_priors_restated.pair_e 1.3e-15, pair_J -> H 4.2e-13 / B 1.3e-13 (2pi: 2.2e-12 / 7.9e-13)
       smooth_restated.between 6.7e-16, between_jacobian 1.2e-15 per entry
   (the 1e-13 of the plain H and B is reduced_system.jr_inv's closed form at residual angles of 1e-4 .. 1e-2, where 1/t^2 - (1 + cos t)/(2 t sin t)
   cancels eight digits.)  Bars: four times those figures.
4. The bars of the GPU tests: the reference's quantities evaluated in float64 numpy by the stable closed forms (rotation_reference.*_terms64,
   mp-free) against the mp values over the WHOLE list.  Worst distance per site, class and quantity (e absolute, J per entry, H and B scaled
   as rotation_reference.distances, cost relative), measured here:
       prior    plain  e 7.1e-15  J 3.7e-15  H 2.6e-15  B 1.5e-14  cost 1.0e-14      2pi  e 1.3e-15  J 7.9e-16  H 5.3e-14  B 7.4e-14  cost 1.2e-14
       pair     plain  e 7.6e-15  J 3.7e-15  H 3.9e-15  B 2.2e-14  cost 2.4e-14      2pi  e 4.7e-15  J 2.3e-15  H 2.2e-12  B 7.9e-13  cost 3.3e-14
       between  plain  e 2.4e-15  J 1.3e-15  H 2.0e-15  B 3.9e-15  cost 8.0e-16
   (e peaks on the generic side of the near-pi switch, where theta / (2 sin theta) = 10.6 multiplies the rounding of Q; "2pi" are the cases
   with a pose vector within 1e-3 of a full turn, where J_l(w) is nearly singular and the scaled measure that much more sensitive.)
   rotation_edge_cases.F64_WORST records them rounded up; the test fails if a recorded figure is more than a factor of two from what this
   machine measures (numpy's sin / cos / arctan2 differ by an ulp between builds).  The GPU bar is 8 x the recorded figure.
"""
import numpy as np
import pytest

import pair_priors_restated as ppr
import reduced_system as rs
import rotation_edge_cases as ec
import rotation_reference as rr
import smooth_restated as sr

M = rr.M


def _hat(w):
    z = M.mpf(0)
    return [[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]]


def _poly(I, a, K, b):
    K2 = rr.mat_mul(K, K)
    return [[I[i][j] + a * K[i][j] + b * K2[i][j] for j in range(3)] for i in range(3)]


_I = [[M.mpf(int(i == j)) for j in range(3)] for i in range(3)]


def jl_mp(w):
    t2 = sum(v * v for v in w)
    t = M.sqrt(t2)
    if t < M.mpf("1e-3"):
        a, b = M.mpf(1) / 2 - t2 / 24 + t2 * t2 / 720 - t2 ** 3 / 40320, M.mpf(1) / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880
    else:
        a, b = (1 - M.cos(t)) / t2, (t - M.sin(t)) / (t2 * t)
    return _poly(_I, a, _hat(w), b)


def jr_inv_mp(phi):
    t2 = sum(v * v for v in phi)
    t = M.sqrt(t2)
    if t < M.mpf("1e-3"):
        k = M.mpf(1) / 12 + t2 / 720 + t2 * t2 / 30240 + t2 ** 3 / 1209600
    else:
        k = 1 / t2 - (1 + M.cos(t)) / (2 * t * M.sin(t))
    return _poly(_I, M.mpf(1) / 2, _hat(phi), k)


def test_exp_of_log_is_the_identity_map():
    worst = M.mpf(0)
    for c in ec.prior_cases():
        Q = rr.mat_mul(rr.mat_t(rr.exp(rr.mpv(c.poses[1][:3]))), rr.exp(rr.mpv(c.poses[0][:3])))
        Q2 = rr.exp(rr.log(Q))
        worst = max(worst, max(abs(Q[i][j] - Q2[i][j]) for i in range(3) for j in range(3)))
    # exactly a half turn: both signs of the axis are the same rotation
    Q = [[M.mpf(-1), M.mpf(0), M.mpf(0)], [M.mpf(0), M.mpf(1), M.mpf(0)], [M.mpf(0), M.mpf(0), M.mpf(-1)]]
    phi = rr.log(Q)
    assert phi[1] == M.pi and phi[0] == 0 and phi[2] == 0
    Q2 = rr.exp(phi)
    worst = max(worst, max(abs(Q[i][j] - Q2[i][j]) for i in range(3) for j in range(3)))
    print("exp(log Q) - Q: %s" % M.nstr(worst, 3))
    assert worst < M.mpf("1e-40")


def test_log_matches_scipy_at_generic_angles():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(200):
        w = rng.standard_normal(3)
        w *= rng.uniform(0.05, 3.0) / np.linalg.norm(w)
        R = rr.to_numpy(rr.exp(rr.mpv(w)))
        got = np.array([float(v) for v in rr.log(rr.exp(rr.mpv(w)))])
        worst = max(worst, np.abs(got - Rotation.from_matrix(R).as_rotvec()).max(), np.abs(got - w).max())
    print("log vs scipy: %.2e" % worst)
    assert worst < 1e-13          # (scipy's own float64 rounding at angles up to 3.0)


def test_differenced_jacobian_is_the_closed_form():
    worst = M.mpf(0)
    for c in ec.prior_cases()[::7]:
        x6, xp = rr.mpv(c.poses[0]), rr.mpv(c.poses[1])
        J = rr.jacobian(rr.prior_e, [x6], [xp])
        phi = rr.prior_e(x6, xp)[:3]
        Mref = rr.mat_mul(jr_inv_mp(phi), rr.mat_t(jl_mp(x6[:3])))
        for i in range(6):
            for j in range(6):
                want = Mref[i][j] if i < 3 and j < 3 else M.mpf(int(i == j))
                worst = max(worst, abs(J[i][j] - want))
    print("differenced J - closed form: %s" % M.nstr(worst, 3))
    assert worst < M.mpf("1e-20")


def _upd(d, k, v):
    d[k] = max(d.get(k, 0.0), float(v))


def test_restatements_agree_below_three_radians():
    got = {}
    for c in ec.prior_cases():
        if c.theta >= 3.0:
            continue
        r = ec.prior_reference()[c.name]
        g = ec.group(c)
        e, J = rs.prior_e(*c.poses), rs.prior_J(*c.poses)
        de, dH, dB, _ = rr.distances(e, J.T @ c.info @ J, -J.T @ c.info @ e, r.cost, r)
        _upd(got, "prior e", de); _upd(got, "prior H " + g, dH); _upd(got, "prior B " + g, dB)
    for c in ec.pair_cases():
        if c.theta >= 3.0:
            continue
        r = ec.pair_reference()[c.name]
        g = ec.group(c)
        e = ppr.pair_e(*c.poses)
        J = np.hstack(ppr.pair_J(*c.poses))
        de, dH, dB, _ = rr.distances(e, J.T @ c.info @ J, -J.T @ c.info @ e, r.cost, r)
        _upd(got, "pair e", de); _upd(got, "pair H " + g, dH); _upd(got, "pair B " + g, dB)
    cases, has, ref = ec.synthetic_between()
    for c, h, r in zip(cases, has, ref):
        if c.theta >= 3.0:
            continue
        J, e = sr.between_jacobian(c.poses[0], c.poses[1], c.poses[2] if h else None)
        _upd(got, "between e", np.abs(e - r.e).max()); _upd(got, "between J", np.abs(J - r.J).max())
    print("restatements:", "  ".join("%s %.2e" % kv for kv in sorted(got.items())))
    bars = {"prior e": 1.4e-15, "prior H plain": 3.2e-13, "prior B plain": 1.3e-13, "prior H 2pi": 5.4e-14, "prior B 2pi": 2.1e-14,
            "pair e": 1.4e-15, "pair H plain": 4.2e-13, "pair B plain": 1.3e-13, "pair H 2pi": 2.2e-12, "pair B 2pi": 7.9e-13,
            "between e": 6.7e-16, "between J": 1.3e-15}
    assert set(got) == set(bars)
    for k, v in got.items():
        assert v <= 4 * bars[k], (k, v, bars[k])


def _measure(site):
    got = {}
    if site == "prior":
        items = [(c, ec.prior_reference()[c.name], rr.prior_terms64(c.poses[0], c.poses[1], c.info)) for c in ec.prior_cases()]
    elif site == "pair":
        items = [(c, ec.pair_reference()[c.name], rr.pair_terms64(c.poses[0], c.poses[1], c.poses[2], c.info)) for c in ec.pair_cases()]
    else:
        cases, has, ref = ec.synthetic_between()
        items = [(c, r, rr.pair_terms64(c.poses[0], c.poses[1], c.poses[2] if h else None, np.eye(6), between=True)) for c, h, r in zip(cases, has, ref)]
    for c, r, f in items:
        de, dH, dB, dc = rr.distances(f.e, f.H, f.B, f.cost, r)
        g = got.setdefault(ec.group(c), {})
        for k, v in (("e", de), ("J", np.abs(f.J - r.J).max()), ("H", dH), ("B", dB), ("cost", dc)):
            _upd(g, k, v)
    return got


@pytest.mark.parametrize("site", ["prior", "pair", "between"])
def test_float64_figures_behind_the_gpu_bars(site):
    got = _measure(site)
    assert set(got) == set(ec.F64_WORST[site])
    for g, fig in sorted(got.items()):
        print("%s %s: %s" % (site, g, "  ".join("%s %.2e (recorded %.1e)" % (k, v, ec.F64_WORST[site][g][k]) for k, v in fig.items())))
        for k, v in fig.items():
            rec = ec.F64_WORST[site][g][k]
            assert 0.5 * rec <= v <= 2.0 * rec, (site, g, k, v, rec)


def test_the_case_list_is_what_it_says():
    """every residual angle of a case is its intended one to 1e-15 (the inputs are rounded once), no case sits on the wrong side of a switch of
    csrc/so3.hpp, the near-pi cases take all three pivots and both signs, and the 'nearest' cases are within 2e-16 of a half turn"""
    pivots, signs = set(), set()
    for cases, ref in ((ec.prior_cases(), ec.prior_reference()), (ec.pair_cases(), ec.pair_reference())):
        for c in cases:
            r = ref[c.name]
            if "nearest" in c.name:
                assert 0 < M.pi - r.angle_mp < 4e-16, (c, r.angle)      # (pi - fl(pi) = 1.2e-16, plus the rounding of fl(pi n)'s entries)
                continue
            assert abs(r.angle - c.theta) < 1e-15, (c, r.angle)
            for sw in (1e-4, 1e-2, ec.SWITCH_PI):
                assert (r.angle < sw) == (c.theta < sw)
            if c.theta > 3.0:
                n = r.e[:3] / r.angle
                p = int(np.argmax(n * n))
                pivots.add(p)
                signs.add(bool(n[p] < 0))
    assert pivots == {0, 1, 2} and signs == {False, True}
