"""Relative pose priors without a GPU: the numpy restatement's analytic Jacobians against central differences, a pair
with a root end against the pose prior, every validation error of aar_problem_constraints_validate names its entry, the appended struct
fields are size-versioned, aar_relative_pose against numpy, the CLI parses its switches.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aar
from conftest import PKG, load_golden
from pair_priors_restated import pair_e, pair_J, pair_J_numeric, pair_terms, relative_pose
from reduced_system import prior_e, rodrigues, slot_col, so3_log

NEW = ("aar_problem_num_pair_priors", "aar_problem_eval_pair_priors", "aar_relative_pose")
ANGLES = (1e-9, 1e-6, 1e-3, 0.3, 1.0, 2.0, 2.5)


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _case(rng, ang):
    """two poses and a prior whose residual rotation is `ang`"""
    xa = np.r_[_unit(rng) * rng.uniform(0.1, 2.0), rng.standard_normal(3)]
    xb = np.r_[_unit(rng) * rng.uniform(0.1, 2.0), rng.standard_normal(3)]
    Rab = rodrigues(xa[:3]).T @ rodrigues(xb[:3])
    Rrel = Rab @ rodrigues(ang * _unit(rng)).T   # R_rel^T R_ab = Exp(ang u)
    xrel = np.r_[so3_log(Rrel), rodrigues(xa[:3]).T @ (xb[3:] - xa[3:]) + 0.05 * rng.standard_normal(3)]
    return xa, xb, xrel


def test_entry_points_are_exported():
    lib = C.CDLL(aar.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n) and n in aar.SYMBOLS
    assert hasattr(aar.Problem, "eval_pair_priors") and hasattr(aar, "relative_pose")
    # include/aar.h layouts: pair prior = 3 int32 (+pad) + 42 doubles; the constraints grow by int32 (+pad) + pointer behind `priors`
    assert C.sizeof(aar.CPairPrior) == 16 + 42 * 8
    assert C.sizeof(aar.CConstraintsV2) == C.sizeof(aar.CConstraints) + 16
    assert aar.CConstraintsV2.n_pair_priors.offset == C.sizeof(aar.CConstraints)
    assert aar.CConstraintsV2.priors.offset == aar.CConstraints.priors.offset


@pytest.mark.parametrize("ang", ANGLES)
def test_analytic_jacobians_match_central_differences(ang):
    rng = np.random.default_rng(int(ang * 1e9) + 1)
    xa, xb, xrel = _case(rng, ang)
    e = pair_e(xa, xb, xrel)
    assert abs(np.linalg.norm(e[:3]) - ang) < 1e-12 + 1e-9 * ang
    Ja, Jb = pair_J(xa, xb, xrel)
    Na, Nb = pair_J_numeric(xa, xb, xrel)
    assert np.abs(Ja - Na).max() < 1e-6 * max(np.abs(Na).max(), 1.0), np.abs(Ja - Na).max()
    assert np.abs(Jb - Nb).max() < 1e-6 * max(np.abs(Nb).max(), 1.0), np.abs(Jb - Nb).max()
    # the blocks the model says are zero
    assert not Ja[:3, 3:].any() and not Jb[:3, 3:].any() and not Jb[3:, :3].any()


def test_pair_with_a_root_end_is_the_pose_prior():
    rng = np.random.default_rng(5)
    for ang in ANGLES:
        _, xb, xrel = _case(rng, ang)
        assert np.array_equal(pair_e(np.zeros(6), xb, xrel), prior_e(xb, xrel))


def test_terms_skip_fixed_ends():
    ds, _ = load_golden("g2_small")
    rng = np.random.default_rng(6)
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker]
    x = ds.x_full
    P = 6 * (ds.num_cams - 1 + ds.num_markers - 1 + ds.num_frames)
    pairs = [("marker", ds.root_marker, fm[0], np.zeros(6), np.eye(6)), ("marker", fm[1], fm[0], 0.1 * rng.standard_normal(6), 2 * np.eye(6))]
    H, B, cost, touched = pair_terms(ds, x, pairs, P, fixed=[("marker", fm[1])])
    c0, c1 = slot_col(ds, "marker", fm[0]), slot_col(ds, "marker", fm[1])
    assert set(touched) == {(c0, c0)} and cost > 0
    assert not H[c1:c1 + 6].any() and not H[:, c1:c1 + 6].any() and not B[c1:c1 + 6].any()
    assert np.allclose(H, H.T) and np.linalg.eigvalsh(H[c0:c0 + 6, c0:c0 + 6]).min() > 0


def test_relative_pose_matches_numpy():
    rng = np.random.default_rng(7)
    for _ in range(20):
        xa = np.r_[_unit(rng) * rng.uniform(0.0, 3.0), rng.standard_normal(3)]
        xb = np.r_[_unit(rng) * rng.uniform(0.0, 3.0), rng.standard_normal(3)]
        got, ref = aar.relative_pose(xa, xb), relative_pose(xa, xb)
        assert np.abs(rodrigues(got[:3]) - rodrigues(ref[:3])).max() < 1e-12
        assert np.abs(got[3:] - ref[3:]).max() < 1e-12
        # a pair that is where it should be has no residual
        assert np.abs(pair_e(xa, xb, got)).max() < 1e-12
    assert np.array_equal(aar.relative_pose(xa, xa)[3:], np.zeros(3))
    assert aar.lib().aar_relative_pose(None, None, None) == aar.AAR_ERR_INVALID


def _pair(kind="marker", a=1, b=2, x6=None, info=None):
    return (kind, a, b, np.zeros(6) if x6 is None else x6, np.eye(6) if info is None else info)


def _invalid(ds, match, **kw):
    with pytest.raises(aar.AarError) as e:
        aar.constraints_validate(ds, **kw)
    assert e.value.code == aar.AAR_ERR_INVALID
    assert match in str(e.value), str(e.value)


def test_valid_pairs_pass():
    ds, _ = load_golden("g2_small")
    fc = [c for c in range(ds.num_cams) if c != ds.root_cam]
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker]
    # a star, a chain, both orientations, a root end, a fixed end, an absolute prior on an end, L = 0 and a rank-deficient L
    aar.constraints_validate(ds, pair_priors=[_pair("marker", fm[0], m) for m in fm[1:]])
    aar.constraints_validate(ds, pair_priors=[_pair("marker", fm[i + 1], fm[i]) for i in range(len(fm) - 1)] + [_pair("camera", fc[1], fc[0])])
    aar.constraints_validate(ds, pair_priors=[_pair("camera", ds.root_cam, fc[0]), _pair("marker", fm[0], ds.root_marker)])
    aar.constraints_validate(ds, fixed_markers=[fm[0]], pair_priors=[_pair("marker", fm[0], fm[1])])
    aar.constraints_validate(ds, priors=[("marker", fm[0], np.zeros(6), np.eye(6))], pair_priors=[_pair("marker", fm[0], fm[1]), _pair("marker", fm[2], fm[0])])
    aar.constraints_validate(ds, pair_priors=[_pair("camera", fc[0], fc[1], info=np.zeros((6, 6)))])
    aar.constraints_validate(ds, pair_priors=[_pair("camera", fc[0], fc[1], info=np.diag([1.0, 1.0, 0.0, 4.0, 0.0, 1.0]))])


def test_every_validation_error_names_its_entry():
    ds, _ = load_golden("g2_small")
    C_, M_ = ds.num_cams, ds.num_markers
    fc = [c for c in range(C_) if c != ds.root_cam]
    fm = [m for m in range(M_) if m != ds.root_marker]
    ok = _pair("marker", fm[0], fm[1])
    _invalid(ds, "pair_priors[0]: kind 7", pair_priors=[(7, 1, 2, np.zeros(6), np.eye(6))])
    _invalid(ds, "pair_priors[1]: marker index_a %d out of range" % M_, pair_priors=[ok, _pair("marker", M_, fm[0])])
    _invalid(ds, "pair_priors[0]: camera index_b -1 out of range", pair_priors=[_pair("camera", fc[0], -1)])
    _invalid(ds, "pair_priors[1]: index_a and index_b are both marker %d" % fm[2], pair_priors=[ok, _pair("marker", fm[2], fm[2])])
    # the same unordered pair twice, in either orientation
    _invalid(ds, "pair_priors[1]: markers %d and %d already have a pair prior (pair_priors[0])" % (fm[0], fm[1]), pair_priors=[ok, ok])
    _invalid(ds, "pair_priors[2]: markers %d and %d already have a pair prior (pair_priors[0])" % (fm[1], fm[0]),
             pair_priors=[ok, _pair("marker", fm[1], fm[2]), _pair("marker", fm[1], fm[0])])
    # ... a camera pair and a marker pair with the same indices are different pairs
    aar.constraints_validate(ds, pair_priors=[_pair("camera", 1, 2), _pair("marker", 1, 2)])
    # both ends fixed: root + fixed index, two fixed indices, a switched-off group
    _invalid(ds, "pair_priors[0]: cameras %d and %d are both fixed" % (ds.root_cam, fc[0]), fixed_cams=[fc[0]], pair_priors=[_pair("camera", ds.root_cam, fc[0])])
    _invalid(ds, "pair_priors[1]: markers %d and %d are both fixed" % (fm[0], fm[1]), fixed_markers=[fm[0], fm[1]], pair_priors=[_pair("marker", fm[2], fm[3]), ok])
    _invalid(ds, "pair_priors[0]: markers %d and %d are both fixed" % (fm[0], fm[1]), pair_priors=[ok], optimize=(True, False, True))
    # information matrices
    asym = np.eye(6)
    asym[0, 1] = 0.5
    for bad in (np.diag([1.0, 1, 1, 1, -1, 1]), -np.eye(6), asym):
        _invalid(ds, "pair_priors[0]: the information matrix", pair_priors=[_pair("marker", fm[0], fm[1], info=bad)])
    # non-finite values
    x6 = np.zeros(6)
    x6[4] = np.inf
    _invalid(ds, "pair_priors[0]: x6_rel[4] is not finite", pair_priors=[_pair("marker", fm[0], fm[1], x6=x6)])
    nan = np.eye(6)
    nan[0, 0] = np.nan
    _invalid(ds, "pair_priors[1]: info[0] is not finite", pair_priors=[ok, _pair("marker", fm[2], fm[3], info=nan)])


def test_struct_size_versioning_of_the_appended_fields():
    ds, _ = load_golden("g2_small")
    bad = [_pair("marker", 99, 1)]
    # a caller whose struct stops behind `priors` (the struct as it was) has no pair priors: they are not read
    aar.constraints_validate(ds, pair_priors=bad, struct_size=C.sizeof(aar.CConstraints))
    _invalid(ds, "null array", pair_priors=bad, struct_size=aar.CConstraintsV2.pair_priors.offset)   # (the count without its array)
    _invalid(ds, "pair_priors[0]", pair_priors=bad, struct_size=C.sizeof(aar.CConstraintsV2))
    # a null array with a count
    cds = ds.as_c()
    d = aar.CProblemDesc()
    aar.lib().aar_problem_desc_from_dataset(C.byref(cds), C.byref(d))
    k = aar.CConstraintsV2()
    k.struct_size = C.sizeof(k)
    k.n_pair_priors = 1
    assert aar.lib().aar_problem_constraints_validate(C.byref(d), C.byref(k)) == aar.AAR_ERR_INVALID
    assert "null array" in aar.lib().aar_last_error().decode()
    k.n_pair_priors = -1
    assert aar.lib().aar_problem_constraints_validate(C.byref(d), C.byref(k)) == aar.AAR_ERR_INVALID
    assert aar.lib().aar_problem_num_pair_priors(None) == 0
    x = np.zeros(8)
    assert aar.lib().aar_problem_eval_pair_priors(None, x.ctypes.data_as(C.POINTER(C.c_double)), None, None) == aar.AAR_ERR_INVALID


def test_bad_pairs_are_reported_before_any_device_is_looked_for():
    ds, _ = load_golden("g2_small")
    with pytest.raises(aar.AarError) as e:
        aar.Problem(ds, pair_priors=[_pair("marker", 1, 1)])
    assert e.value.code == aar.AAR_ERR_INVALID


def _cli(*args):
    exe = os.path.join(PKG, "aar_find_solution")
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_parses_the_switches_and_builds_the_chain(tmp_path):
    folder = str(tmp_path / "s2")
    assert _cli("--synth", 2, folder).returncode == 0
    ds = aar.solution_read(os.path.join(folder, "initial.solution"))
    sol = os.path.join(folder, "initial.solution")
    # a chain over all cameras and all markers: one pair less than entities, per kind; the pair of two held ends is left out
    for kinds, n in (("both", ds.num_cams - 1 + ds.num_markers - 1), ("cams", ds.num_cams - 1), ("markers", ds.num_markers - 1)):
        r = _cli(folder, 0.05, "x", "-from-initial", "-relative-prior-solution", sol, "-relative-kinds", kinds, "-relative-sigma-deg", 0.5, "-relative-sigma-m", 0.002)
        line = "constraints: %d relative pose prior(s) from %s (%s, sigma 0.5 deg, 0.002 m)" % (n, sol, kinds)
        assert line in r.stdout, r.stdout + r.stderr
        if aar.device_count() == 0:
            assert r.returncode == 2 and "no CPU path" in r.stderr
    free_c = [int(ds.cam_ids[c]) for c in range(ds.num_cams) if c != ds.root_cam]
    assert ds.root_cam == 0   # (the chain's first camera pair is then (root, first free camera))
    r = _cli(folder, 0.05, "x", "-from-initial", "-fix-cams", free_c[0], "-relative-prior-solution", sol, "-relative-kinds", "cams")
    assert "constraints: %d relative pose prior(s)" % (ds.num_cams - 2) in r.stdout, r.stdout + r.stderr
    for bad in (("-relative-kinds", "frames"), ("-relative-sigma-deg", "0"), ("-relative-sigma-m", "x")):
        r = _cli(folder, 0.05, "x", "-from-initial", *bad)
        assert r.returncode != 0 and "Usage" in r.stdout, bad
    r = _cli(folder, 0.05, "x", "-from-initial", "-relative-prior-solution", str(tmp_path / "missing.solution"))
    assert r.returncode == 5 and "cannot read the relative prior solution" in r.stderr
