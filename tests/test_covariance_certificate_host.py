"""The covariance certificate (tests/covariance_certificate.py) on the host: its bars are ones that plain float64 meets with room, and that a
wrong factor gather, a wrong block, a wrong frame sum or a wrong mask does not meet.  H comes from the oracle; no GPU.

Reference within the bar: on every case of the device module (CASES below) two independent float64 routes stay at or below 1/8 of the bars (a)
and (b): np.linalg.inv of the whole H over its rows with an unknown, and a restatement of the device's method -- tile LDL^T of the Schur
complement summed in reverse frame order, X = L^-1 by block rows of 32, X^T D^-1 X, the frame formula with np.linalg.solve for V_f^-1.
Measured (entity ratio, frame ratio; worst of both routes):

    tile sweep nT = 1 .. 14        8.4e-6, 9.6e-4      gauge rows 1.2e-6, 8.6e-5; groups off 1.6e-6, 4.5e-4; fixed 2.0e-6, 5.7e-5
    unseen marker                  2.3e-5, 4.9e-4      empty frame 1.1e-6, 1.4e-4; roots-only frame 3.0e-6, 5.2e-4
    small frames                   2.5e-6, 1.1e-3      wide frames 8.7e-6, 4.3e-4
    small frames with intrinsics   2.3e-7, 3.6e-2      the intrinsics fixture, whole 1.9e-8, 1.9e-2; cut 9.9e-9, 2.6e-2
    Huber 2.2e-8, 1.7e-3           priors with a fixed camera 5.4e-6, 1.5e-3
    g2_small 1.4e-9, 4.4e-3        config 3 whole 4.7e-7, 1.3e-3      config-5-shaped slice 1.7e-6, 1.2e-4

The entity ratios are 1e-6 of the bar because every frame's share of M carries kappa_f = cond_2(V_f) (30 .. 70 on the synthetic sets, 9 000 where
a frame sees one camera and one marker, 13 000 in g2_small) and |Sigma| M |Sigma| is a worst case over the signs.  The frame ratios of np.linalg.inv
are largest with intrinsics, where a frame's block of H^-1 comes out of an inverse with focal lengths in pixels.

Planted faults fail and are located: a 96-column block of L taken from the unfactored system (the wrong k_cov_gather branch; located by its
extent -- the blocks still inside their bars are exactly those with both entities beyond that block column), a transposed 6 x 6 block of Sigma
(the worst block), one (entity, frame) pair left out of S (the block where the error carried back to S is largest), and in one frame: W rounded
to fp32, the sum without the transpose term, with diagonal weight 1, with a held entity's columns left in G (the worst frame).

What the bar does not see: a relative error in one block of Sigma below eps* = bar_ab / |Sigma*_ab| (covariance_certificate.block_resolution).
For the middle entity's diagonal block eps* is 1.1e-6 on the one-tile set and 1.6e-5 on the fourteen-tile set; for its block with the largest
partner 1.8e-6 and 3.2e-5.  The flat 1e-7 of tests/test_gpu_covariance.py stays: on its sets it sees smaller errors than these bars do.  An error of 4 eps* fails and is located, one of eps* / 4 passes; both are tests.
"""
import re

import numpy as np
import pytest

import covariance_certificate as cc
import direct_cases as dc
import oracle_lib as ol
from covariance_cases import CASES, case_keywords, x0_of
from reduced_system import prior_terms


_SYS = {}


def _setup(name):
    if name not in _SYS:
        make, kw = CASES[name]
        ds = make()
        opt, intr, hub, fixed, pri = case_keywords(ds, kw, np.asarray(ds.x_full, dtype=np.float64))
        o = ol.Oracle(ds, optimize=opt, with_huber=hub, intrinsics=intr)
        x = x0_of(ds, intr)
        H, B = o.normal_equations(x, res_mode=ol.RES_F32)
        Hp = prior_terms(ds, x, pri, len(B))[0] if pri else None
        _SYS.clear()                                       # (one system at a time: the large ones are 30 MB apiece)
        _SYS[name] = (ds, cc.CovSystem(ds, H, opt, intr, Hp=Hp, **fixed))
    return _SYS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_conditioning_premise_and_two_float64_routes_within_an_eighth_of_the_bars(name):
    ds, cs = _setup(name)
    # premise: H over its rows with an unknown is positive definite and far from singular -- a set that drifts singular fails here, not the kernel
    idx = np.r_[cs.ent[cs.live], cs.frame_idx]
    Hl = cs.H[np.ix_(idx, idx)]
    assert np.linalg.eigvalsh(Hl)[0] > 0, name
    if CASES[name][1].get("intrinsics"):
        # (focal lengths and principal points are in pixels, poses in radians and metres: cond_2 is not invariant under that choice of units, the
        # unpivoted LDL^T and the componentwise bars are -- so the premise is stated for H with a unit diagonal)
        d = 1 / np.sqrt(np.diag(Hl))
        Hl = Hl * np.outer(d, d)
    ev = np.linalg.eigvalsh(Hl)
    assert ev[0] > 0 and ev[-1] / ev[0] < 1e10, (name, ev[0], ev[-1] / ev[0])
    s1, f1 = cc.dense_inverse_route(cs)
    s2 = cc.device_method(cs)
    f2 = cc.frames_by_solves(cs, s2)
    for how, sg, fr in (("np.linalg.inv of H", s1, f1), ("the device's method in float64", s2, f2)):
        a = cc.certify_entity(cs, sg, "%s, %s" % (name, how))
        b = cc.certify_frames(cs, sg, fr, "%s, %s" % (name, how))
        print("%s, %s: entity %.3e, frames %.3e (premise %.1e, cond_2(H) %.2e)" % (name, how, a["ratio"], b["ratio"], a["premise"], ev[-1] / ev[0]))
        assert a["ratio"] <= 0.125 and b["ratio"] <= 0.125, (name, how, a, b)
        assert len(b["certified"]) == len(cs.frames_live)


def test_the_masked_cases_have_the_rows_they_are_named_after():
    ds, cs = _setup("worklist_unseen")
    k = [b[:2] for b in cs.blocks].index(("marker", 7))
    o = cs.blocks[k][2]
    assert not cs.live[o:o + 6].any() and cs.live.sum() == cs.n - 6
    ds, cs = _setup("empty_frame")
    assert list(set(range(cs.nF)) - set(cs.frames_live)) == [5]
    ds, f = dc.roots_only_frame(dc.worklist_ds(60))
    ds, cs = _setup("roots_only_frame")
    k = list(cs.frames_live).index(f)
    assert cs.kf[k] == 2 and not cs.rs.W64[:, k, :].any()
    ref, _ = cc.frame_reference(cs, cc.device_method(cs))
    assert np.array_equal(ref[k], cs.rs.Vinv[k])                      # Sigma_ff = V_f^-1
    ds, cs = _setup("intrinsics")
    for kind, idx_, o, sz in cs.blocks:
        assert list(cs.live[o:o + sz]) == ([True] * 4 + [False] * 5 if kind == "intrinsics" else [True] * 6) or not cs.live[o:o + sz].any()
    assert sum(b[0] == "intrinsics" for b in cs.blocks) == ds.num_cams
    ds, cs = _setup("fixed_3")
    assert (~cs.live).sum() == 18
    assert dc.frame_entity_counts(dc.small_frames_ds())[:5] == dc.SMALL_TARGETS
    ds, cs = _setup("small_frames_intr")
    assert set(dc.SMALL_TARGETS_INTRINSICS) <= set(dc.frame_entity_counts(ds, intrinsics=True)) and set(dc.SMALL_TARGETS_INTRINSICS) <= set(cs.kf)


def test_the_wide_product_is_a_product():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((70, 90)) * 10.0 ** rng.integers(-6, 6, (70, 1))
    B = rng.standard_normal((90, 50)) * 10.0 ** rng.integers(-6, 6, (1, 50))
    Pw, off = cc.matmul_wide(A, B)
    ref = A.astype(np.longdouble) @ B.astype(np.longdouble)
    assert np.all(np.abs(np.asarray(Pw - ref, dtype=np.float64)) <= off + 90 * float(np.finfo(np.longdouble).eps) * (np.abs(A) @ np.abs(B)))
    assert np.all(off <= 2.0 ** -58 * (np.abs(A).max(axis=1, keepdims=True) * np.abs(B).max(axis=0, keepdims=True)) * 90)      # 32 x below float64


# ---- planted faults ----
def _entity_rows(cs, k):
    return slice(cs.blocks[k][2], cs.blocks[k][2] + cs.blocks[k][3])


def test_a_block_of_l_from_the_unfactored_system_fails_and_is_located():
    ds, cs = _setup("sweep5")
    A, _ = cc.reduce_reverse(cs.rs)
    L, D = cc.block_ldl(A)
    ti, tj = 3, 2
    L[96 * ti:96 * ti + 96, 96 * tj:96 * tj + 96] = A[96 * ti:96 * ti + 96, 96 * tj:96 * tj + 96]      # (k_ldl_trsm's column read before the chain ran)
    with pytest.raises(cc.CovarianceCertificateError, match="worst block") as ei:
        cc.certify_entity(cs, cc.device_method(cs, L, D), "wrong gather branch")
    # located by its extent (the factor is off by |D|: too far for the first-order backward error): L_ij enters X_KB for B <= j, K >= i, and
    # Sigma_AB = sum_K X_KA^T D^-1 X_KB -- the blocks still within their bars are exactly those with both entities beyond tile j
    beyond = np.array([b[2] >= 96 * (tj + 1) for b in cs.blocks])
    assert np.array_equal(ei.value.ratios <= 1.0, np.outer(beyond, beyond)), str(ei.value)


def _worst(ei, which="worst"):
    m = re.search({"worst": "worst", "backward": "largest in"}[which] + r" block: \((\w+) (\d+), (\w+) (\d+)\)", str(ei.value))
    return (m.group(1), int(m.group(2))), (m.group(3), int(m.group(4)))


def test_a_transposed_block_fails_and_is_located():
    ds, cs = _setup("sweep5")
    sg = cc.device_method(cs)
    i = len(cs.blocks) // 2
    j = max((j for j in range(len(cs.blocks)) if j != i), key=lambda j: np.linalg.norm(sg[_entity_rows(cs, i), _entity_rows(cs, j)]))
    blk = sg[_entity_rows(cs, i), _entity_rows(cs, j)].copy()
    sg[_entity_rows(cs, i), _entity_rows(cs, j)] = blk.T
    sg[_entity_rows(cs, j), _entity_rows(cs, i)] = blk
    with pytest.raises(cc.CovarianceCertificateError, match="worst block") as ei:
        cc.certify_entity(cs, sg, "transposed")
    assert set(_worst(ei)) == {cs.blocks[i][:2], cs.blocks[j][:2]}, str(ei.value)


def test_a_pair_left_out_of_s_fails_and_is_located():
    ds, cs = _setup("sweep5")
    rs = cs.rs
    i = len(cs.blocks) // 2
    oa = cs.blocks[i][2]
    fr = np.nonzero((rs.W64[oa:oa + 6] != 0).any(axis=(0, 2)))[0]
    f = fr[len(fr) // 2]
    Wf = rs.W64[:, f, :]
    W0 = Wf.copy()
    W0[oa:oa + 6] = 0.0
    A = rs.A64 + Wf @ rs.Vinv[f] @ Wf.T - W0 @ rs.Vinv[f] @ W0.T
    sg = np.linalg.inv(A)
    sg[cs.nan_pattern()] = np.nan
    with pytest.raises(cc.CovarianceCertificateError, match="worst block") as ei:
        cc.certify_entity(cs, sg, "pair left out")
    assert cs.blocks[i][:2] in _worst(ei, "backward"), str(ei.value)


def _frame_fault(cs, kind):
    """(entity covariance, frame blocks with frame f wrong, f)"""
    rs = cs.rs
    sg = cc.device_method(cs)
    fr = cc.frames_by_solves(cs, sg)
    s0 = np.nan_to_num(sg)
    bid = np.zeros(cs.n, int)
    for k in range(len(cs.blocks)):
        bid[_entity_rows(cs, k)] = k
    k = rs.F // 2
    G = rs.Vinv[k] @ rs.W64[:, k, :].T
    if kind == "fp32_w":
        G32 = rs.Vinv[k] @ rs.W32[:, k, :].T
        blk = rs.Vinv[k] + G32 @ s0 @ G32.T
    elif kind == "no_transpose_term":
        blk = rs.Vinv[k] + G @ (s0 * (bid[:, None] <= bid[None, :])) @ G.T
    elif kind == "diagonal_weight_1":
        blk = rs.Vinv[k] + G @ (s0 * (1 + (bid[:, None] == bid[None, :]))) @ G.T
    else:
        assert kind == "held_columns_left"
        he = np.nonzero(rs.held_e)[0]
        Wh = cs.H[np.ix_(cs.ent[he], cs.frame_idx.reshape(-1, 6)[k])]         # the coupling the restatement zeroed; S^-1 of an identity row is 1
        assert Wh.any(), "the frame does not see a held entity"
        Gh = rs.Vinv[k] @ Wh.T
        blk = rs.Vinv[k] + G @ s0 @ G.T + Gh @ Gh.T
    f = int(cs.frames_live[k])
    fr[f] = blk
    return sg, fr, f


@pytest.mark.parametrize("kind", ["fp32_w", "no_transpose_term", "diagonal_weight_1", "held_columns_left"])
def test_a_wrong_frame_sum_fails_and_is_located(kind):
    ds, cs = _setup("fixed_3" if kind == "held_columns_left" else "sweep5")
    sg, fr, f = _frame_fault(cs, kind)
    cc.certify_entity(cs, sg, kind)
    with pytest.raises(cc.CovarianceCertificateError, match="worst frame: %d " % f):
        cc.certify_frames(cs, sg, fr, kind)


def test_a_block_of_an_empty_frame_and_a_wrong_nan_pattern_fail():
    ds, cs = _setup("empty_frame")
    sg = cc.device_method(cs)
    fr = cc.frames_by_solves(cs, sg)
    fr[5] = 0.0
    with pytest.raises(cc.CovarianceCertificateError, match="frame 5 has no detections"):
        cc.certify_frames(cs, sg, fr, "empty frame")
    ds, cs = _setup("worklist_unseen")
    sg = cc.device_method(cs)
    sg[~np.isfinite(sg)] = 0.0
    with pytest.raises(cc.CovarianceCertificateError, match="NaN pattern"):
        cc.certify_entity(cs, sg, "no NaN")


# ---- what the bar does not see ----
@pytest.mark.parametrize("tiles,diag_range,off_range", [(1, (5e-7, 3e-6), (5e-7, 3e-6)), (14, (8e-6, 4e-5), (8e-6, 5e-5))])
def test_the_smallest_block_error_the_bar_sees(tiles, diag_range, off_range):
    ds, cs = _setup("sweep%d" % tiles)
    s0 = cc.device_method(cs)
    i = len(cs.blocks) // 2
    j = max((j for j in range(len(cs.blocks)) if j != i), key=lambda j: np.linalg.norm(s0[_entity_rows(cs, i), _entity_rows(cs, j)]))
    for (a, b), rng_ in (((i, i), diag_range), ((i, j), off_range)):
        eps = cs.block_resolution(a, b)
        print("sweep%d block (%d, %d): eps* = %.3e" % (tiles, a, b, eps))
        assert rng_[0] <= eps <= rng_[1], eps
        for fac, fails in ((4.0, True), (0.25, False)):
            sg = s0.copy()
            sg[_entity_rows(cs, a), _entity_rows(cs, b)] *= 1 + fac * eps
            if a != b:
                sg[_entity_rows(cs, b), _entity_rows(cs, a)] *= 1 + fac * eps
            if fails:
                with pytest.raises(cc.CovarianceCertificateError, match="worst block") as ei:
                    cc.certify_entity(cs, sg, "scaled")
                assert set(_worst(ei)) == {cs.blocks[a][:2], cs.blocks[b][:2]}
            else:
                assert cc.certify_entity(cs, sg, "scaled")["ratio"] <= 1.0
