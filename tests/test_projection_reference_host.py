"""The independent reference of tests/projection_reference.py, itself checked on the CPU -- and, through it, the formula that the oracle and
the kernels share.

1. The reference's 8 x 18 block against mpmath at 60 digits (central difference, step 1e-20) on one observation per edge angle.
   Measured (edge_dataset(theta), the observation of camera 1 / marker 1 / frame 1, relative to each row's largest entry):
   1.3e-16 at exactly 0, 1e-20, 1e-17, 3e-16 and 0.01 - 1e-6; 2.5e-16 at 1e-9, 1e-5, 0.01 + 1e-6; 3.2e-16 .. 4.2e-16 at pi - 1e-9, pi,
   pi + 1e-9 and 2 pi - 1e-3.  Largest 4.2e-16; bar 1e-13.
2. The oracle's analytic path (Oracle.jacobian / normal_equations, JAC_ANALYTIC: left_jacobian_so3 + analytic_blocks, the restatement
   of csrc/geom.hpp) against the reference, on every golden fixture and every edge data set (25: twelve angles, each on camera 1 +
   marker 1 + frame 1 and on all markers at once, and exactly 0 with zero translation), both residual modes, Huber and intrinsics
   included, each group switched off in turn, and g1_cfg2 with six entities moved to theta + 2 pi.  Bars are the project's own
   (tests/test_gpu_parity.py): H 1e-12 of max|H|, B 1e-11 of max|B|, residual rows 1e-9 px in double mode; each input must stay 10x
   inside them.  Measured, largest over all inputs:
   J 4.4e-15 of each row's largest entry (edge 0.01 + 1e-6; the fixtures 1.7e-15), H 4.2e-15 (the same edge; fixtures 2.0e-15),
   B 2.5e-13 in double mode (edge 0, zero translation; the projection at u ~ 1000 px is good to 2e-13 px and B sees that) and 4.4e-15 in
   float mode, rows 1.4e-12 px (g1_cfg2_retry; the edge sets 4.6e-13).
   Float mode without Huber: the reference's rows are BIT-EQUAL to the oracle's on every input (asserted); with Huber they differ by one
   rounding (4.4e-16), so bit-equality of Huber rows stays with the oracle.
3. The diagonal-scaled measure |H - H_ref|_ij / sqrt(H_ii H_jj) (projection_reference.scaled_error), which max|H| hides the small blocks
   from: largest for the oracle over all these inputs 5.0e-14 (the two edge data sets at theta = 0.01 + 1e-6, where the closed form
   (theta - sin theta) / theta^3 has lost digits to cancellation just above the series switch; everywhere else <= 1.3e-14, g2_small).
   The bar, for oracle and device alike, is 100x that: projection_reference.SCALED_BAR = 5e-12.
"""
import glob
import os

import numpy as np
import pytest

import oracle_lib as ol
import projection_reference as pr
from conftest import GOLDEN, load_golden

H_BAR, B_BAR, ROW_BAR = 1e-12, 1e-11, 1e-9      # tests/test_gpu_parity.py
INSIDE = 10.0                                   # the oracle must sit this far inside each bar on the CPU
MPMATH_BAR = 1e-13


def _fixtures():
    names = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        with np.load(path) as g:
            if "meta" in g.files and "obs_uv" in g.files and "x_full" in g.files:
                names.append(os.path.splitext(os.path.basename(path))[0])
    return names


FIXTURES = _fixtures()
EDGE_CASES = [(th, board, False) for th in pr.EDGE_ANGLES for board in (False, True)] + [(0.0, False, True)]


def _edge_id(case):
    return "theta=%.17g%s%s" % (case[0], "-board" if case[1] else "", "-t0" if case[2] else "")


def _jac_error(o, R, x):
    """largest |J_oracle - J_ref| relative to each row's largest entry, block-wise: the oracle's triplets are scattered into the reference's
    [n, 8, npar] layout through Reference.columns() (no dense 8N x P matrix), and every triplet must land in a column the reference has"""
    rows, cols, vals = o.jacobian(x, jac_mode=ol.JAC_ANALYTIC)
    J, col = R.jacobian_blocks(x)
    n, npar = col.shape
    obs, r8 = rows // 8, rows % 8
    hit = col[obs] == cols[:, None]                          # [nnz, npar]: which parameter of its observation a triplet belongs to
    live = hit.any(axis=1)
    assert live.all() or not np.abs(vals[~live]).any()       # (the five idle intrinsics columns per camera: explicit zeros of the oracle)
    got = np.zeros_like(J)
    np.add.at(got, (obs[live], r8[live], hit[live].argmax(axis=1)), vals[live])
    Jz = np.where((col >= 0)[:, None, :], J, 0.0)
    scale = np.abs(Jz).max(axis=2)
    keep = scale > 0                                         # (a row has no column at all where root sees root with the frames switched off)
    assert not got[~keep].any() and keep.any()
    return float((np.abs(got - Jz).max(axis=2)[keep] / scale[keep]).max())


def _check(ds, x, name, groups=True):
    """the oracle against the reference on one input, through all switches; returns the measured maxima"""
    m = dict(J=0.0, H=0.0, B=0.0, B32=0.0, rows=0.0, scaled=0.0)
    combos = [(hub, intr, (True, True, True)) for hub in (None, 1.5) for intr in (False, True)]
    if groups:
        combos += [(None, False, opt) for opt in ((False, True, True), (True, False, True), (True, True, False))]
    for hub, intr, opt in combos:
        o = ol.Oracle(ds, optimize=opt, with_huber=hub is not None, huber_delta=hub if hub is not None else 10.0, intrinsics=intr)
        R = pr.Reference(ds, optimize=opt, intrinsics=intr, huber_delta=hub)
        assert R.P == o.num_vars
        m["J"] = max(m["J"], _jac_error(o, R, x))
        for res in (pr.RES_F32, pr.RES_F64):
            H, B, ss = R.normal_equations(x, res)
            Ho, Bo = o.normal_equations(x, jac_mode=ol.JAC_ANALYTIC, res_mode=res)
            r, ro = R.residuals(x, res), o.residuals(x, res_mode=res)
            eH = np.abs(Ho - H).max() / np.abs(H).max()
            eB = np.abs(Bo - B).max() / np.abs(B).max()
            er = np.abs(ro - r).max()
            es = pr.scaled_error(Ho, H)
            print("%s huber=%s intr=%d opt=%s res=%d: H %.2e B %.2e rows %.2e scaled %.2e" % (name, hub, intr, opt, res, eH, eB, er, es))
            assert eH < H_BAR / INSIDE and eB < B_BAR / INSIDE and er < ROW_BAR / INSIDE, (name, hub, intr, opt, res, eH, eB, er)
            assert es < pr.SCALED_BAR, (name, hub, intr, opt, res, es)
            assert abs(ss - float((ro ** 2).sum())) <= 1e-12 * ss
            if res == pr.RES_F32 and hub is None:
                assert np.array_equal(r, ro), (name, intr, opt)            # float-faithful rows: the same bits
            m["H"] = max(m["H"], eH); m["B" if res == pr.RES_F64 else "B32"] = max(m["B" if res == pr.RES_F64 else "B32"], eB)
            m["rows"] = max(m["rows"], er); m["scaled"] = max(m["scaled"], es)
    print("%s: measured %s" % (name, {k: "%.2e" % v for k, v in m.items()}))
    return m


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_analytic_path_on_golden_fixtures(name):
    ds, _ = load_golden(name)
    m = _check(ds, ds.x_full, name)
    assert m["J"] < 1e-12


@pytest.mark.parametrize("case", EDGE_CASES, ids=_edge_id)
def test_oracle_analytic_path_on_edge_poses(case):
    ds = pr.edge_dataset(case[0], board=case[1], zero_translation=case[2])
    m = _check(ds, ds.x_full, _edge_id(case))
    assert m["J"] < 1e-12


def test_oracle_analytic_path_in_the_other_chart():
    # theta + 2 pi for a fixture's own theta: the same rotations (the rows do not move), another chart (the columns do)
    ds, _ = load_golden("g1_cfg2")
    C, M = ds.num_cams, ds.num_markers
    rows = [0, 2, C - 1, C - 1 + 3, C - 1 + M - 1, C - 1 + M - 1 + 5]        # two cameras, two markers, two frames
    x = pr.other_chart(ds.x_full, rows)
    R = pr.Reference(ds)
    assert np.abs(R.residuals(x) - R.residuals(ds.x_full)).max() < 1e-9
    H0, _, _ = R.normal_equations(ds.x_full)
    H1, _, _ = R.normal_equations(x)
    assert np.abs(H1 - H0).max() > 1e-3 * np.abs(H0).max()                   # (it IS another chart)
    _check(ds, x, "g1_cfg2 + 2 pi")


def test_h_is_continuous_across_the_series_switch():
    # the two sides of |w| = 1e-2 (where J_l goes from its series to the closed form): same data set up to the angle, so H moves by
    # O(2e-6) of itself at most -- and the ORACLE's H moves by the same amount as the reference's, to the bar
    lo, hi = pr.edge_dataset(0.01 - 1e-6), pr.edge_dataset(0.01 + 1e-6)
    assert np.array_equal(lo.obs_frame, hi.obs_frame) and np.array_equal(lo.obs_marker, hi.obs_marker)
    jump = {}
    for who in ("ref", "oracle"):
        Hs = []
        for ds in (lo, hi):
            Hs.append(pr.Reference(ds).normal_equations(ds.x_full)[0] if who == "ref"
                      else ol.Oracle(ds).normal_equations(ds.x_full, jac_mode=ol.JAC_ANALYTIC, res_mode=ol.RES_F64)[0])
        jump[who] = Hs[1] - Hs[0]
    scale = np.abs(pr.Reference(lo).normal_equations(lo.x_full)[0]).max()
    assert np.abs(jump["ref"]).max() / scale < 1e-3
    assert np.abs(jump["oracle"] - jump["ref"]).max() / scale < H_BAR


def _mp_block(mp, vec18, K, h, step):
    """d(projection) / d(18 pose parameters) of one observation by a central difference at mpmath's working precision"""
    def rod(w):
        t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        W = mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        if t2 == 0:
            return mp.eye(3)
        t = mp.sqrt(t2)
        return mp.eye(3) + (mp.sin(t) / t) * W + ((1 - mp.cos(t)) / t2) * (W * W)

    def proj(v):
        Rc, Rm, Rf = rod(v[0:3]), rod(v[6:9]), rod(v[12:15])
        tc, tm, tf = mp.matrix(v[3:6]), mp.matrix(v[9:12]), mp.matrix(v[15:18])
        out = []
        for sx, sy in ((-1, 1), (1, 1), (1, -1), (-1, -1)):
            X = mp.matrix([sx * h, sy * h, 0])
            p = Rc.T * (Rf * (Rm * X + tm) + tf - tc)
            q = K * p
            out += [q[0] / q[2], q[1] / q[2]]
        return out

    G = np.zeros((8, 18))
    for k in range(18):
        vp, vm = list(vec18), list(vec18)
        vp[k] = vp[k] + step
        vm[k] = vm[k] - step
        a, b = proj(vp), proj(vm)
        for r in range(8):
            G[r, k] = float((a[r] - b[r]) / (2 * step))
    return G


@pytest.mark.parametrize("theta", pr.EDGE_ANGLES, ids=lambda t: "theta=%.17g" % t)
def test_reference_block_against_mpmath(theta):
    import mpmath as mp
    mp.mp.dps = 60
    ds = pr.edge_dataset(theta)
    R = pr.Reference(ds)
    score = (R.oc_ == 1).astype(int) + (R.om_ == 1) + (R.of_ == 1)
    o = int(np.argmax(score))
    assert score[o] >= 2
    G = R.blocks(ds.x_full, slice(o, o + 1))[0]
    cam, mk, fr = R.entity_vectors(ds.x_full)
    vec = [mp.mpf(float(v)) for v in np.concatenate([cam[R.oc_[o]], mk[R.om_[o]], fr[R.of_[o]]])]
    K = mp.matrix(np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 3, 3)[R.oc_[o]].tolist())
    Gm = _mp_block(mp, vec, K, mp.mpf(R.h), mp.mpf("1e-20"))
    err = float((np.abs(G - Gm).max(axis=1) / np.abs(Gm).max(axis=1)).max())
    print("theta %.17g, observation %d (%d of camera 1 / marker 1 / frame 1): reference vs mpmath %.2e" % (theta, o, score[o], err))
    assert err < MPMATH_BAR


def test_builder_refuses_what_it_cannot_realise():
    cams = np.zeros((2, 6)); mks = np.zeros((2, 6)); frs = np.zeros((1, 6))
    frs[0, 3:] = [0, 0, -3.0]                                    # behind the root camera
    with pytest.raises(ValueError, match="projective pole"):
        pr.build_dataset(cams, mks, frs, [0], [0], [0])
    frs[0, 3:] = [0, 0, 3.0]
    with pytest.raises(ValueError, match="ordered by frame"):
        pr.build_dataset(cams, mks, np.tile(frs, (2, 1)), [1, 0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="out of range"):
        pr.build_dataset(cams, mks, frs, [0], [2], [0])
