"""The direct chain's certificate (tests/direct_certificate.py) on the host: the bar is one that plain float64 meets with room, and that a wrong
Schur complement, factorisation or back-substitution does not meet.  H, B come from the oracle; no GPU.

Reference within the bar: two independent float64 solves of every launch-shape case of tests/direct_cases.py -- np.linalg.solve on the restated
A, and an unpivoted block LDL^T in 96-row tiles on the Schur complement summed in reverse frame order -- each with a frame part that does not use
the restatement's inverses (np.linalg.solve on V_f, reverse order) must stay at ratio <= 1/8 in (a) and (c), at mu = 1e-3 max diag H and
mu = max diag H.  Worst reference ratio measured per family (either solve, either mu):

    tile sweep nT = 1 .. 14           6.8e-4      gauge rows 4.4e-4, switched-off groups 8.2e-4, fixed 2.8e-4
    work lists (3 .. 60 frames)       1.1e-3      wide frames (k_schur<3>)                     1.8e-4
    MFMA frame lists, dense counts    6.6e-4      Huber 4.0e-4, intrinsics 4.4e-5, priors 3.0e-4
    frame part, all families          5.3e-5

(medians 2e-5 .. 3e-4.  At the small damping kappa_f ~ 30 .. 50 weights the frames' shares and the bar is ~ 1e5 u |A| |d_s|.)

Sensitivity, on the two-tile and the seven-tile set of the sweep at both dampings.  A step from a system with one (entity, frame) pair left out of
the Schur sum, with the damping missing from one diagonal entry, or with one block of A stored transposed fails (a) by factors of 1e6 .. 1e11, and
(b) names the entity; these take the middle entity of the z order and its largest partner block.  A RELATIVE error in one block is another matter:
the bar resolves an error eps in block (a, b) only from eps* = bar / |(A_ab d_b, A_ba d_a)| on (direct_certificate.block_resolution).  For the middle
entity's block with its largest partner eps* is, per family (median, worst; small damping | large damping):

    tile sweep           5.5e-8, 8.9e-7 | 1.4e-9, 5.3e-6      gauge rows, fixed    6e-8, 8e-8 | 7e-10, 1e-9
    work lists           3.8e-9, 6.9e-9 | 4e-11, 6e-11        wide frames          5e-8, 6e-8 | 9e-10, 1e-9
    MFMA lists, dense    4e-9, 8e-9     | 7e-11, 1e-10        Huber, priors        8e-9       | 1e-10

so the issue's 1 + 1e-9 is below the resolution of an ordinary block at the small damping and in the larger sweeps: a 1e-9 error there PASSES the
certificate.  Two tests state this: "scaled" applies 1 + 1e-9 to the most visible block of the system (the largest share of the residual), the only
kind of block in which the bar sees 1e-9 on every set -- ratios 4.5 and 30 at two tiles, 1.75 and 1.37 at seven; "scaled_at_resolution" applies
4 eps* to the middle entity's block, which must fail and be located.  With the slack as the Frobenius product |A|_F ulp |z_s| the seven-tile
"scaled" case at mu = max diag H reached 0.76; the row-wise slack of the certificate is what brings it over 1.
"""
import numpy as np
import pytest

import direct_cases as dc
import oracle_lib as ol
from conftest import load_golden
from direct_certificate import DirectCertificateError, block_ldl_solve, block_resolution, build_system, certify_direct, entity_blocks, reduce_reverse
from reduced_system import prior_terms, slot_col

MUS = (1e-3, 1.0)          # times max diag H


def _x0(ds, intrinsics):
    x = np.asarray(ds.x_full, dtype=np.float64)
    if not intrinsics:
        return x
    K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 9)
    d = np.asarray(ds.dist_coeffs, dtype=np.float64).reshape(-1, 5)
    return np.concatenate([x, np.concatenate([np.stack([K[:, 0], K[:, 2], K[:, 4], K[:, 5]], axis=1), d], axis=1).reshape(-1)])


def _priors(ds, x):
    rng = np.random.default_rng(3)
    pr = []
    for c in range(ds.num_cams):
        if c != ds.root_cam:
            col = slot_col(ds, "camera", c)
            A = rng.standard_normal((6, 6))
            pr.append(("camera", c, x[col:col + 6] + np.r_[0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)], 1e3 * (A @ A.T + 6 * np.eye(6))))
    return pr


def _fixed(ds):
    fc = [c for c in range(ds.num_cams) if c != ds.root_cam][:2]
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker][3:4]
    return dict(fixed_cams=fc, fixed_markers=fm)


CASES = {}
for _nT in range(1, 15):
    CASES["sweep%d" % _nT] = (lambda nT=_nT: dc.sweep_ds(nT), {})
for _c in (15, 16, 34):
    CASES["gauge_c%d" % _c] = (lambda c=_c: dc.gauge_ds(c, 3), {})
for _t in (3, 5):
    CASES["cams_off_%d" % _t] = (lambda t=_t: dc.gauge_ds(16, t), dict(optimize=(False, True, True)))
    CASES["markers_off_%d" % _t] = (lambda t=_t: dc.gauge_ds(16, t), dict(optimize=(True, False, True)))
    CASES["fixed_%d" % _t] = (lambda t=_t: dc.gauge_ds(16, t), "fixed")
for _F in (3, 8, 9, 60):
    CASES["worklist_F%d" % _F] = (lambda F=_F: dc.worklist_ds(F), {})
CASES["worklist_unseen"] = (lambda: dc.without_pairs(dc.worklist_ds(60), 7, 11), {})
for _m in (84, 92):
    CASES["wide_%d" % _m] = (lambda m=_m: dc.wide_frames_ds(m), {})
for _F in (1, 2, 3, 4, 5, 8, 9):
    CASES["mfma_F%d" % _F] = (lambda F=_F: dc.mfma_frames_ds(F), {})
for _e in (30, 31, 32):
    CASES["dense_%d" % (_e + 1)] = (lambda e=_e: dc.dense_count_ds(e), {})
CASES["huber"] = (lambda: load_golden("g1_cfg2_huber")[0], dict(with_huber=True))
CASES["intrinsics"] = (lambda: load_golden("g1_cfg2_intr")[0], dict(intrinsics=True))
CASES["priors"] = (lambda: load_golden("g1_cfg3_cut")[0], "priors")


def _setup(name):
    make, kw = CASES[name]
    ds = make()
    extra = {}
    if kw == "fixed":
        kw, extra = {}, _fixed(ds)
    pri = kw == "priors"
    if pri:
        kw = {}
    opt, intr = kw.get("optimize", (True, True, True)), kw.get("intrinsics", False)
    o = ol.Oracle(ds, optimize=opt, with_huber=kw.get("with_huber", False), intrinsics=intr)
    x = _x0(ds, intr)
    H, B = o.normal_equations(x, res_mode=ol.RES_F32)
    Hp = Bp = None
    if pri:
        Hp, Bp, _ = prior_terms(ds, x, _priors(ds, x), len(B))
    md = float(np.diag(H).max())
    blocks = entity_blocks(ds, opt, intr)
    z0 = o.extract_z(x)
    systems = [build_system(ds, H, B, m * md, opt, intr, Hp=Hp, Bp=Bp, **extra) for m in MUS]
    return ds, blocks, z0, systems


def _backsub_by_solves(rs, d_s):
    """the frame part without the restatement's inverses: V_f x = g_f - W_f^T d_s by np.linalg.solve, last frame first, the sum over the entities
    in reverse order"""
    df = np.zeros((rs.F, 6))
    for f in range(rs.F - 1, -1, -1):
        df[f] = np.linalg.solve(rs.V[f], rs.gf[f] - rs.W64[::-1, f, :].T @ d_s[::-1])
    return df


@pytest.mark.parametrize("name", list(CASES))
def test_two_float64_solves_stay_within_an_eighth_of_the_bar(name):
    ds, blocks, z0, systems = _setup(name)
    for rs in systems:
        A, b = reduce_reverse(rs)
        for how, d_s in (("np.linalg.solve", rs.solve_s()), ("block LDL^T, reverse frame order", block_ldl_solve(A, b))):
            d = rs.assemble(d_s, _backsub_by_solves(rs, d_s))
            out = certify_direct(rs, d, z0 + d, blocks, "%s mu %.3g %s" % (name, rs.mu, how))
            assert out["ratio"] <= 0.125 and out["frame_ratio"] <= 0.125, (name, rs.mu, how, out)


def test_the_block_ldl_is_a_solve():
    rs = _setup("sweep3")[3][0]
    A, b = reduce_reverse(rs)
    np.testing.assert_allclose(A, rs.A64, rtol=0, atol=1e-12 * np.abs(rs.A64).max())
    x = block_ldl_solve(A, b)
    np.testing.assert_allclose(x, np.linalg.solve(A, b), rtol=0, atol=1e-9 * np.abs(x).max())


# ---- sensitivity ----
_SENS = {}


def _sens(tiles):
    if tiles not in _SENS:
        _SENS[tiles] = _setup("sweep%d" % tiles)
    return _SENS[tiles]


def _mutated(rs, blocks, kind, z0):
    """(A', b', the entities the mutation touches) -- the entity is the middle block of the z order; its partner the block with the largest share"""
    A, b = rs.A64.copy(), rs.b64.copy()
    bi = len(blocks) // 2
    oa = blocks[bi][2]
    if kind == "pair_left_out":
        fr = np.nonzero((rs.W64[oa:oa + 6] != 0).any(axis=(0, 2)))[0]
        f = fr[len(fr) // 2]
        Wf = rs.W64[:, f, :]
        W0 = Wf.copy()
        W0[oa:oa + 6] = 0.0
        A += Wf @ rs.Vinv[f] @ Wf.T - W0 @ rs.Vinv[f] @ W0.T
        b += (Wf - W0) @ rs.Vinv[f] @ rs.gf[f]
        return A, b, [blocks[bi][:2]]
    if kind == "no_damping":
        A[oa + 2, oa + 2] -= rs.mu
        return A, b, [blocks[bi][:2]]
    d0 = rs.solve_s()
    if kind == "scaled":
        # the off-diagonal block (a, b) whose share of the residual, A_ab d_b and A_ba d_a, is largest: the most visible one
        best, bi, bj = 0.0, 0, 0
        for i in range(len(blocks)):
            for j in range(i):
                oi, oj = blocks[i][2], blocks[j][2]
                v = np.hypot(np.linalg.norm(A[oi:oi + 6, oj:oj + 6] @ d0[oj:oj + 6]), np.linalg.norm(A[oj:oj + 6, oi:oi + 6] @ d0[oi:oi + 6]))
                if v > best:
                    best, bi, bj = v, i, j
        oa, ob = blocks[bi][2], blocks[bj][2]
        A[oa:oa + 6, ob:ob + 6] *= 1 + 1e-9
        A[ob:ob + 6, oa:oa + 6] *= 1 + 1e-9
        return A, b, [blocks[bi][:2], blocks[bj][:2]]
    bj = max((j for j in range(len(blocks)) if j != bi), key=lambda j: np.linalg.norm(A[oa:oa + 6, blocks[j][2]:blocks[j][2] + 6]))
    ob = blocks[bj][2]
    if kind == "scaled_at_resolution":
        # the middle entity's block with its largest partner -- chosen like the other mutations' -- off by four times what the bar resolves there
        eps = 4 * block_resolution(rs, d0, rs.split(z0)[0], blocks, bi, bj)
        A[oa:oa + 6, ob:ob + 6] *= 1 + eps
        A[ob:ob + 6, oa:oa + 6] *= 1 + eps
        return A, b, [blocks[bi][:2], blocks[bj][:2]]
    assert kind == "transposed"
    blk = A[oa:oa + 6, ob:ob + 6].copy()
    A[oa:oa + 6, ob:ob + 6] = blk.T
    A[ob:ob + 6, oa:oa + 6] = blk
    return A, b, [blocks[bi][:2], blocks[bj][:2]]


@pytest.mark.parametrize("mu_i", [0, 1])
@pytest.mark.parametrize("tiles", [2, 7])
@pytest.mark.parametrize("kind", ["pair_left_out", "scaled", "scaled_at_resolution", "no_damping", "transposed"])
def test_a_wrong_reduced_step_fails_and_is_located(kind, tiles, mu_i):
    ds, blocks, z0, systems = _sens(tiles)
    rs = systems[mu_i]
    A, b, touched = _mutated(rs, blocks, kind, z0)
    d_s = np.linalg.solve(A, b)
    d = rs.assemble(d_s, rs.backsub(d_s))
    with pytest.raises(DirectCertificateError, match="worst block row") as ei:
        certify_direct(rs, d, z0 + d, blocks, kind)
    assert any("worst block row: %s %d " % t in str(ei.value) for t in touched), (str(ei.value), touched)


@pytest.mark.parametrize("mu_i", [0, 1])
@pytest.mark.parametrize("tiles", [2, 7])
def test_a_frame_back_substituted_through_fp32_blocks_fails(tiles, mu_i):
    ds, blocks, z0, systems = _sens(tiles)
    rs = systems[mu_i]
    d_s = rs.solve_s()
    df = rs.backsub(d_s)
    f = rs.F // 2
    df[f] = rs.backsub(d_s, w32=True)[f]
    d = rs.assemble(d_s, df)
    with pytest.raises(DirectCertificateError, match="back-substitution: frame %d " % f):
        certify_direct(rs, d, z0 + d, blocks, "fp32 W in frame %d" % f)


def test_a_moved_fixed_entity_fails():
    ds, blocks, z0, systems = _setup("fixed_3")
    rs = systems[0]
    d = rs.exact_step()
    i = int(np.nonzero(rs.held_e)[0][0])
    d[rs.ent[i]] = 1e-300
    with pytest.raises(DirectCertificateError, match="fixed entity"):
        certify_direct(rs, d, z0 + d, blocks, "fixed")


# ---- the data sets reach the shapes they are named after ----
def test_the_data_sets_reach_their_launch_shapes():
    for nT in range(1, 15):
        ds = dc.sweep_ds(nT)
        assert dc.tiles_of(ds) == nT and 6 * (ds.num_cams + ds.num_markers) == 96 * nT - 18
    for cams, row in ((16, 96), (15, 90), (34, 204)):       # the root marker's rows: first of tile 1, last of tile 0, inside tile 2
        ds = dc.gauge_ds(cams, 3)
        assert dc.tiles_of(ds) == 3 and 6 * (ds.num_cams + ds.root_marker) == row
    assert dc.tiles_of(dc.gauge_ds(16, 5)) == 5
    for F in (3, 8, 9, 60):
        ds = dc.worklist_ds(F)
        assert dc.tiles_of(ds) == 2 and ds.num_frames == F and min(dc.frame_entity_counts(ds)) > 0
    fpm = dc.frames_per_marker(dc.without_pairs(dc.worklist_ds(60), 7, 11))
    assert fpm[7] == 0 and fpm[11] == 1 and min(fpm[:7] + fpm[8:11] + fpm[12:]) > 1
    for markers, mfma_default in ((84, False), (92, True)):
        ds = dc.wide_frames_ds(markers)
        kf = dc.frame_entity_counts(ds)
        assert max(kf) > 64 and min(kf) < 30 and any(30 < k < 60 for k in kf) and any(60 < k <= 64 for k in kf), kf
        assert (ds.num_cams + ds.num_markers >= 96) == mfma_default
    for F in (1, 2, 3, 4, 5, 8, 9):
        ds = dc.mfma_frames_ds(F)
        assert dc.tiles_of(ds) == 2 and ds.num_frames == F and min(dc.frame_entity_counts(ds)) > 0
    for dense in (31, 32, 33):                                # with the pseudo entity g_f: padded to 32, 32, 64
        assert dc.seen_entities(dc.dense_count_ds(dense - 1)) + 1 == dense
