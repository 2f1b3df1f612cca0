"""The case list of the rotation-log certificates -- TEST INFRASTRUCTURE ONLY.  Built once per session (functools.lru_cache), shared by
tests/test_rotation_reference_host.py and tests/test_gpu_rotation_edges.py, never modified by a test.

A case is a residual rotation Exp(theta n) and the float64 poses that produce it.  The partner vector is built in mp
(rotation_reference.partner_vector) and rounded to float64 once; the reference is then evaluated at those float64 numbers, so the residual
angle of a case is whatever the rounded inputs give, within ~1e-16 of theta.  Every switch of csrc/so3.hpp is approached from both sides at
a distance (1e-7 of 1e-4, 1e-6 of 1e-2 and of acos(-0.99)) that the rounding of the inputs cannot cross.

    RESIDUAL_ANGLES   16 angles: zero, below any epsilon, the two sides of so3_log's series switch (1e-4), of so3_jr_inv's (1e-2), generic angles,
                      the two sides of so3_log's near-pi switch (cos = -0.99), and pi - 1e-3 .. pi - 1e-12
    "nearest"         a seventeenth: the identity against fl(pi n) -- as close to a half turn as float64 goes (pi - fl(pi) = 1.2e-16)
    AXES              every coordinate axis (one pivot, two exact-zero components) and one of them negated; the ties of the pivot selection
                      d0 >= d1 >= d2; one almost-zero component; two generic axes whose largest component is negative (sign -1)
    VECTOR_ANGLES     the classes of the poses' own rotation vectors, from projection_reference.EDGE_ANGLES
"""
import functools

import numpy as np

import rotation_reference as rr
from projection_reference import EDGE_ANGLES

PI = float(np.pi)
SWITCH_PI = float(np.arccos(-0.99))
RESIDUAL_ANGLES = [0.0, 1e-20, 1e-9, 1e-4 - 1e-7, 1e-4 + 1e-7, 1e-2 - 1e-6, 1e-2 + 1e-6, 1.0, 2.5, SWITCH_PI - 1e-6, SWITCH_PI + 1e-6, 3.1,
                   PI - 1e-3, PI - 1e-6, PI - 1e-9, PI - 1e-12]
NEAR_PI = [a for a in RESIDUAL_ANGLES if a > 3.0]          # the angles of so3_log's third branch
AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, -1, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1e-9, 1, 0), (-0.8, 0.3, 0.5), (0.2, -0.7, -0.6),
        (0.4, 0.5, -0.77)]
VECTOR_ANGLES = [0.0, 1e-20, 0.01 - 1e-6, 0.01 + 1e-6, PI, PI + 1e-9, 2 * PI - 1e-3]
assert all(a in EDGE_ANGLES for a in VECTOR_ANGLES)
assert len(RESIDUAL_ANGLES) == 16


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _spd(rng):
    A = rng.standard_normal((6, 6))
    return A @ A.T + 6.0 * np.eye(6)


def _nearest(axis):
    n = np.asarray(axis, dtype=np.float64)
    return PI * (n / np.linalg.norm(n))


class Case:
    """name, theta (intended), axis, poses (a tuple of float64 6-vectors, per site), info (unit-scale SPD 6x6)"""

    def __init__(self, name, theta, axis, poses, info):
        self.name, self.theta, self.axis, self.poses, self.info = name, theta, axis, tuple(np.asarray(p, dtype=np.float64) for p in poses), info

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def prior_cases():
    """poses = (x6, xp).  Classes "own k": the entity's vector at VECTOR_ANGLES[k] about a random axis, the prior's vector its partner;
    "prior 0" / "prior pi": the PRIOR's vector zero / a half turn and the entity's vector the partner; "nearest": w = 0, w_p = fl(pi n)."""
    rng = np.random.default_rng(1234)
    out = []
    for ia, th in enumerate(RESIDUAL_ANGLES):
        for ix, ax in enumerate(AXES):
            for k, va in enumerate(VECTOR_ANGLES):
                w = _unit(rng) * va
                t = 0.3 * rng.standard_normal(3)
                wp = rr.partner_vector(w, th, ax, "ref")
                out.append(Case("prior a%d x%d own%d" % (ia, ix, k), th, ax, (np.r_[w, t], np.r_[wp, t + 0.05 * rng.standard_normal(3)]), _spd(rng)))
            for tag, va in (("prior0", 0.0), ("priorpi", PI)):
                wp = _unit(rng) * va
                t = 0.3 * rng.standard_normal(3)
                w = rr.partner_vector(wp, th, ax, "own")
                out.append(Case("prior a%d x%d %s" % (ia, ix, tag), th, ax, (np.r_[w, t], np.r_[wp, t + 0.05 * rng.standard_normal(3)]), _spd(rng)))
    for ix, ax in enumerate(AXES):
        t = 0.3 * rng.standard_normal(3)
        out.append(Case("prior nearest x%d" % ix, PI, ax, (np.r_[np.zeros(3), t], np.r_[_nearest(ax), t + 0.05 * rng.standard_normal(3)]), _spd(rng)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pair_cases():
    """poses = (xa, xb, xrel) of a relative prior.  Class k: end b's vector at VECTOR_ANGLES[k], end a's at another class (all 49 combinations
    occur), the prior's vector w_rel = log(R_ab Exp(theta n)^T); "rel0": w_rel = 0 (the commonest relative prior) and end b the partner of end a;
    "nearest": w_a = w_rel = 0, w_b = fl(pi n)."""
    rng = np.random.default_rng(4321)
    out = []
    nv = len(VECTOR_ANGLES)
    for ia, th in enumerate(RESIDUAL_ANGLES):
        for ix, ax in enumerate(AXES):
            for k, vb in enumerate(VECTOR_ANGLES):
                wa = _unit(rng) * VECTOR_ANGLES[(k + ia + ix) % nv]
                wb = _unit(rng) * vb
                ta, tb = 0.3 * rng.standard_normal(3), 0.3 * rng.standard_normal(3)
                Rab = rr.mat_mul(rr.mat_t(rr.exp(rr.mpv(wa))), rr.exp(rr.mpv(wb)))
                wrel = rr.partner_vector(Rab, th, ax, "ref")
                trel = rr.to_numpy(rr.exp(rr.mpv(wa))).T @ (tb - ta) + 0.05 * rng.standard_normal(3)
                out.append(Case("pair a%d x%d own%d" % (ia, ix, k), th, ax, (np.r_[wa, ta], np.r_[wb, tb], np.r_[wrel, trel]), _spd(rng)))
            wa = _unit(rng) * VECTOR_ANGLES[(ia + ix) % nv]
            ta, tb = 0.3 * rng.standard_normal(3), 0.3 * rng.standard_normal(3)
            wb = rr.partner_vector(wa, th, ax, "own")
            trel = rr.to_numpy(rr.exp(rr.mpv(wa))).T @ (tb - ta) + 0.05 * rng.standard_normal(3)
            out.append(Case("pair a%d x%d rel0" % (ia, ix), th, ax, (np.r_[wa, ta], np.r_[wb, tb], np.r_[np.zeros(3), trel]), _spd(rng)))
    for ix, ax in enumerate(AXES):
        ta, tb = 0.3 * rng.standard_normal(3), 0.3 * rng.standard_normal(3)
        out.append(Case("pair nearest x%d" % ix, PI, ax, (np.r_[np.zeros(3), ta], np.r_[_nearest(ax), tb], np.r_[np.zeros(3), tb - ta + 0.05 * rng.standard_normal(3)]),
                        _spd(rng)))
    return tuple(out)


def is_near_pi(case):
    return case.theta > 3.0


def between_rel(za, zb, theta, axis, rng):
    """the expected motion (rvec, t) that leaves a residual Exp(theta n) between the poses za, zb: w_rel = log(R_ab Exp(-theta n)),
    dt = t_b - t_a - (a few centimetres)"""
    Rab = rr.mat_mul(rr.mat_t(rr.exp(rr.mpv(za[:3]))), rr.exp(rr.mpv(zb[:3])))
    return np.r_[rr.partner_vector(Rab, theta, axis, "ref"), zb[3:] - za[3:] - 0.05 * rng.standard_normal(3)]


NULL_REL_ANGLES = [3.1, PI - 1e-6, PI - 1e-9]      # pairs WITHOUT an expected motion whose poses really differ by this much


def between_track(z):
    """(z' [F, 6], rel [F - 1, 6], has_rel [F - 1], cases): a track for the between factor, one pair per case.  z [>= F, 6] supplies the poses;
    pair f = (z'_f, z'_f+1).  The first 16 x 12 pairs keep the poses of z and carry the residual in rel[f]; the last three pairs have no
    expected motion (has_rel False, rel row zero -- a track either has rel_motion or not, so the caller passes their zero rows or splits the
    call): their second pose IS the first one turned by NULL_REL_ANGLES about a generic axis.  cases[f].poses = (za, zb, rel or zeros)."""
    rng = np.random.default_rng(777)
    z = np.array(z, dtype=np.float64)
    specs = [(th, ax) for th in RESIDUAL_ANGLES for ax in AXES]
    F = len(specs) + len(NULL_REL_ANGLES) + 1
    assert len(z) >= F, (len(z), F)
    z = z[:F].copy()
    rel = np.zeros((F - 1, 6))
    has = np.zeros(F - 1, dtype=bool)
    cases = []
    for f, (th, ax) in enumerate(specs):
        rel[f] = between_rel(z[f], z[f + 1], th, ax, rng)
        has[f] = True
    for n, th in enumerate(NULL_REL_ANGLES):          # (behind the last pair with a motion, in order: each starts from the pose the one before left)
        f = len(specs) + n
        z[f + 1, :3] = rr.partner_vector(z[f, :3], th, AXES[9 + n], "own")
        z[f + 1, 3:] = z[f, 3:] + 0.05 * rng.standard_normal(3)
    for f in range(F - 1):
        th, ax = specs[f] if f < len(specs) else (NULL_REL_ANGLES[f - len(specs)], AXES[9 + f - len(specs)])
        cases.append(Case("between f%d a%d x%d%s" % (f, RESIDUAL_ANGLES.index(th) if has[f] else -1, AXES.index(ax), "" if has[f] else " null"), th, ax,
                          (z[f], z[f + 1], rel[f]), None))
    return z, rel, has, cases


def synthetic_track(F, seed=99):
    """poses of an object three units in front of the root camera, moving by a few hundredths of a radian and a few centimetres a frame"""
    rng = np.random.default_rng(seed)
    z = np.zeros((F, 6))
    z[0] = np.r_[_unit(rng) * 0.5, 0.0, 0.0, 3.0]
    for f in range(1, F):
        z[f, :3] = rr.partner_vector(z[f - 1, :3], 0.03 * (1 + rng.random()), _unit(rng), "own")
        z[f, 3:] = z[f - 1, 3:] + 0.03 * rng.standard_normal(3)
    return z


BETWEEN_FRAMES = 16 * len(AXES) + len(NULL_REL_ANGLES) + 1


def between_reference(cases, has, lam_rot, lam_trans):
    """the mp terms of a track's pairs at the information diag(lam_rot x3, lam_trans x3), in pair order"""
    info = np.diag([lam_rot] * 3 + [lam_trans] * 3)
    return [rr.between_terms(c.poses[0], c.poses[1], c.poses[2] if h else None, info) for c, h in zip(cases, has)]


@functools.lru_cache(maxsize=None)
def synthetic_between():
    """(cases, has_rel, reference at unit information) of the synthetic track: what the host test measures the float64 figures on"""
    z, rel, has, cases = between_track(synthetic_track(BETWEEN_FRAMES))
    return cases, has, between_reference(cases, has, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def prior_reference():
    """the mp terms of every prior case at unit information, by case name"""
    return {c.name: rr.prior_terms(c.poses[0], c.poses[1], c.info) for c in prior_cases()}


@functools.lru_cache(maxsize=None)
def pair_reference():
    return {c.name: rr.pair_terms(c.poses[0], c.poses[1], c.poses[2], c.info) for c in pair_cases()}


# ---------------------------------------------------------------- the bars
# The worst distance of the float64 evaluation (rotation_reference.*_terms64) from the mp reference over the whole case list, per call site and
# quantity, as tests/test_rotation_reference_host.py measures it on the CPU (it fails if a figure here is off by more than a factor of two):
# e absolute, J absolute per entry, H and B in rotation_reference.distances' scaled measure, cost relative.  "2pi": the cases with a pose whose
# own rotation vector is within 1e-3 of a full turn, where J_l(w) has two singular values of 1.6e-4 and the scaled measure of H and B is that
# much more sensitive; "plain": all others.  The device is held to FACTOR times these figures: the margin covers another association of the
# 3 x 3 products and a few ulp of the device's sincos / atan2.  Nothing here comes from a device.
F64_WORST = {
    "prior": {"plain": dict(e=7.2e-15, J=3.8e-15, H=2.7e-15, B=1.6e-14, cost=1.1e-14), "2pi": dict(e=1.4e-15, J=7.9e-16, H=5.4e-14, B=7.4e-14, cost=1.2e-14)},
    "pair": {"plain": dict(e=7.7e-15, J=3.8e-15, H=3.9e-15, B=2.2e-14, cost=2.5e-14), "2pi": dict(e=4.7e-15, J=2.4e-15, H=2.2e-12, B=7.9e-13, cost=3.3e-14)},
    "between": {"plain": dict(e=2.4e-15, J=1.4e-15, H=2.0e-15, B=3.9e-15, cost=8.1e-16)},
}
FACTOR = 8.0


def group(case):
    return "2pi" if max(np.linalg.norm(p[:3]) for p in case.poses) > 6.0 else "plain"


def bar(site, case, quantity):
    return FACTOR * F64_WORST[site][group(case)][quantity]
