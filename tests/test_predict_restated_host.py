"""The restatement of the corner covariance (tests/predict_restated.py) on the host: H from the oracle, no GPU.

1. The block route (S^-1, the frame formula, Sigma_fe = -G Sigma_e, the mask rule, complex-step J) against J_full H^-1 J_full^T from
   numpy.linalg.inv of H over its live rows, for every detection and for every (camera, marker) of three frames, in the measure
   |C_a - C_b|_F / s_q, s_q = | |J| |Sigma_q| |J^T| |_F.  The GPU tests hold the device to the project's flat 1e-7 in that measure; here the two
   float64 routes must stay below 1/8 of it.  Measured worst value per case:

       sweep2 2.9e-12          gauge_c16 3.1e-13      cams_off_3 1.1e-13     markers_off_3 4.5e-13    fixed_3 2.0e-13
       worklist_unseen 3.4e-13 empty_frame 1.2e-12    roots_only_frame 4.8e-13   small_frames 4.3e-12 wide_84 2.9e-13
       huber 1.2e-11           priors_fixed 5.2e-13   g2_small 1.6e-8

   with the median of s_q / |C_q| between 280 and 4 000 -- and 2.1e6 on g2_small, the one case whose two float64 routes do not stay below
   1/8 of the flat bar: its conditioning is too poor for a flat bar, so it is left out of the flat-bar GPU test (the certificate covers it).
2. The identities: without priors the leverages tr(C_i) of the problem's own detections sum to P_live within 1e-7 sum s_i and every
   eigenvalue of C_i lies in [-1e-7 s_i, 1 + 1e-7 s_i]; with priors the sum is P_live - tr(H^-1 H_prior).
3. Planted faults (predict_restated.FAULTS) exceed the flat bar: each is a mistake a kernel of this shape can make.
"""
import numpy as np
import pytest

import oracle_lib as ol
import predict_restated as prs
from covariance_cases import CASES, case_keywords, x0_of
from reduced_system import prior_terms

NAMES = ["sweep2", "gauge_c16", "cams_off_3", "markers_off_3", "fixed_3", "worklist_unseen", "empty_frame", "roots_only_frame", "small_frames",
         "wide_84", "huber", "priors_fixed", "g2_small"]
POORLY_CONDITIONED = {"g2_small"}     # measured 1.6e-8 > 1.25e-8, median s_q / |C| = 2e6
FLAT_CASES = [n for n in NAMES if n not in POORLY_CONDITIONED]
_SYS = {}


def setup(name):
    """(ds, x, PredictSystem, Hp or None) of a case, H from the oracle"""
    if name not in _SYS:
        make, kw = CASES[name]
        ds = make()
        opt, intr, hub, fixed, pri = case_keywords(ds, kw, np.asarray(ds.x_full, dtype=np.float64))
        assert not intr
        o = ol.Oracle(ds, optimize=opt, with_huber=hub)
        x = x0_of(ds, False)
        H, B = o.normal_equations(x, res_mode=ol.RES_F32)
        Hp = prior_terms(ds, x, pri, len(B))[0] if pri else None
        _SYS.clear()
        _SYS[name] = (ds, x, prs.PredictSystem(ds, H, opt, Hp=Hp, **fixed), Hp)
    return _SYS[name]


def all_queries(ds):
    return np.concatenate([prs.detection_queries(ds), prs.frame_grid_queries(ds, prs.three_frames(ds))])


def worst_ratio(a, b, s):
    ok = np.isfinite(s)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    return float((np.linalg.norm((a - b)[ok], axis=(1, 2)) / s[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("name", NAMES)
def test_block_route_against_the_dense_inverse(name):
    ds, x, ps, _ = setup(name)
    q = all_queries(ds)
    Cb, s, uv, st = prs.covariances(ps, x, q, "block")
    Cd, sd, _, st2 = prs.covariances(ps, x, q, "dense")
    assert np.array_equal(st, st2)
    w = worst_ratio(Cb, Cd, s)
    defined = st == 0
    canc = float(np.median(s[defined] / np.linalg.norm(Cb[defined], axis=(1, 2))))
    print("%s: %d queries (%d undefined, %d behind), worst |C_block - C_dense| / s_q = %.2e, median s_q / |C| = %.0f"
          % (name, len(q), int(((st & prs.UNDEFINED) != 0).sum()), int(((st & prs.BEHIND) != 0).sum()), w, canc))
    if name in POORLY_CONDITIONED:
        # the two float64 routes themselves differ by more than 1/8 of the flat bar: the cancellation eats six digits here.  The case is left out
        # of the flat-bar GPU test (tests/test_gpu_predict_corners.py: FLAT_CASES); the certificate there, whose bar carries kappa_f, covers it
        assert canc > 1e5, (name, canc)
    else:
        assert w <= prs.FLAT_BAR / 8, (name, w)
    assert defined.sum() >= len(ds.obs_cam) - 1


@pytest.mark.parametrize("name", NAMES)
def test_leverage_identities(name):
    ds, x, ps, Hp = setup(name)
    q = prs.detection_queries(ds)
    C, s, _, st = prs.covariances(ps, x, q, "block")
    assert not st.any(), "a detection makes its triple seen"
    lev = np.trace(C, axis1=1, axis2=2)
    want = float(ps.num_live_vars)
    if Hp is not None:
        want -= float(np.trace(ps.Hinv @ Hp[np.ix_(ps.idx, ps.idx)]))
    print("%s: sum of leverages %.12g, expected %.12g (P_live %d), leverages %.3f .. %.3f" % (name, lev.sum(), want, ps.num_live_vars, lev.min(), lev.max()))
    assert abs(lev.sum() - want) <= prs.FLAT_BAR * s.sum(), (name, lev.sum(), want)
    ev = np.linalg.eigvalsh(0.5 * (C + C.transpose(0, 2, 1)))
    assert (ev.min(axis=1) >= -prs.FLAT_BAR * s).all() and (ev.max(axis=1) <= 1 + prs.FLAT_BAR * s).all(), name
    assert (lev > 0).all() and (lev < 8 + prs.FLAT_BAR * s).all()


def test_the_named_cases_have_the_states_they_are_named_after():
    ds, x, ps, _ = setup("worklist_unseen")
    assert ps.entity_state("marker", 7) == ("unseen",)
    q = np.array([[c, 7, 0] for c in range(ds.num_cams)])
    C, s, uv, st = prs.covariances(ps, x, q)
    assert ((st & prs.UNDEFINED) != 0).all() and np.isnan(C).all() and np.isfinite(uv[(st & prs.BEHIND) == 0]).all()
    ds, x, ps, _ = setup("empty_frame")
    assert ps.frame_state(5) == ("unseen",) and ps.frame_state(4)[0] == "live"
    ds, x, ps, _ = setup("fixed_3")
    from covariance_cases import fixed_of
    fx = fixed_of(ds)
    assert all(ps.entity_state("camera", c) == ("const",) for c in fx["fixed_cams"])
    assert all(ps.entity_state("marker", m) == ("const",) for m in fx["fixed_markers"])
    ds, x, ps, _ = setup("cams_off_3")
    assert all(ps.entity_state("camera", c) == ("const",) for c in range(ds.num_cams))
    # a constant contributes zero, not NaN: a root query is defined
    q = np.array([[ds.root_cam, ds.root_marker, 0]])
    C, s, uv, st = prs.covariances(ps, x, q)
    assert st[0] == 0 and np.isfinite(C).all()


@pytest.mark.parametrize("fault", prs.FAULTS)
def test_planted_faults_exceed_the_bar(fault):
    name = "fixed_3" if fault == "held_identity" else "sweep2"
    ds, x, ps, _ = setup(name)
    q = all_queries(ds)
    if fault == "held_identity":
        from covariance_cases import fixed_of
        held = fixed_of(ds)["fixed_cams"]
        q = q[np.isin(q[:, 0], held)]
        assert len(q)
    Cd, s, _, st = prs.covariances(ps, x, q, "dense")
    Cf, _, _, _ = prs.covariances(ps, x, q, "block", fault=fault)
    ok = st == 0
    r = np.linalg.norm((Cf - Cd)[ok], axis=(1, 2)) / s[ok]
    print("%s on %s: |C_fault - C_dense| / s_q median %.2e, max %.2e" % (fault, name, np.median(r), r.max()))
    assert r.max() > 1e3 * prs.FLAT_BAR, (fault, r.max())
    if fault in ("no_cross", "cross_sign"):
        assert np.median(r) > 0.05            # (the cross blocks decide the answer: an error of the order of s_q itself)


def test_the_certificate_reference_follows_the_blocks_it_is_given():
    # the reference of the GPU certificate (with_device_blocks, certificate_bars) on the host: fed with the restatement's own blocks it returns
    # the block route to the bit; a slot missing from the cross sum is far outside its bars
    ds, x, ps, _ = setup("sweep2")
    q = all_queries(ds)
    ec = ps.Sinv.copy()
    ec[ps.cs.nan_pattern()] = np.nan
    fr = np.full((ds.num_frames, 6, 6), np.nan)
    for k, f in enumerate(ps.cs.frames_live):
        fr[f] = ps.gain(k)[1]
    ref = prs.with_device_blocks(ps, ec, fr)
    Cb, s, _, st = prs.covariances(ps, x, q)
    Cr, s2, _, _ = prs.covariances(ref, x, q)
    assert np.array_equal(Cb, Cr) and np.array_equal(s, s2)
    bars = prs.certificate_bars(ps, q, s)
    assert (bars > 2 * prs.pr.SCALED_BAR * s).all() and (bars < 1e-10 * s).all()
    Cf, _, _, _ = prs.covariances(ps, x, q, fault="skip_slot")
    assert (np.linalg.norm(Cf - Cr, axis=(1, 2)) / bars).max() > 1e6
