"""The float64 restatement of the damped reduced system (tests/reduced_system.py) against the oracle's own damped solve: the reduced solve plus
the frame back-substitution is the step of the oracle's sparse LDL^T (Oracle.damped_solve) on every layout the GPU certificates use -- switched-off
groups, Huber weights, the intrinsics entities, fixed entities.  No GPU."""
import numpy as np
import pytest

import oracle_lib as ol
from conftest import load_golden
from reduced_system import ReducedSystem, held_mask, split_indices


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _x0(ds, intrinsics):
    if not intrinsics:
        return np.asarray(ds.x_full, dtype=np.float64)
    K = np.asarray(ds.cam_mats, dtype=np.float64).reshape(-1, 9)
    d = np.asarray(ds.dist_coeffs, dtype=np.float64).reshape(-1, 5)
    intr = np.concatenate([np.stack([K[:, 0], K[:, 2], K[:, 4], K[:, 5]], axis=1), d], axis=1).reshape(-1)
    return np.concatenate([np.asarray(ds.x_full, dtype=np.float64), intr])


CASES = [("g1_cfg2", {}), ("g1_cfg3_cut", {}), ("g1_cfg2_huber", {"with_huber": True}), ("g1_cfg2_intr", {"intrinsics": True}),
         ("g1_cfg3_cut", {"optimize": (False, True, True)}), ("g1_cfg3_cut", {"optimize": (True, False, True)}),
         ("g1_cfg3_cut", {"optimize": (True, True, False)}), ("g1_cfg2", {"optimize": (False, False, True)})]


@pytest.mark.parametrize("name,kw", CASES)
def test_reduced_solve_and_back_substitution_are_the_oracles_damped_step(name, kw):
    ds, _ = load_golden(name)
    opt = kw.get("optimize", (True, True, True))
    intr = kw.get("intrinsics", False)
    o = ol.Oracle(ds, optimize=opt, with_huber=kw.get("with_huber", False), intrinsics=intr)
    x = _x0(ds, intr)
    H, B = o.normal_equations(x, res_mode=ol.RES_F32)
    ent, fr = split_indices(ds, opt, intr)
    assert len(ent) + len(fr) == len(B)
    for mu in (float(np.diag(H).max()), float(np.diag(H).max()) * 1e-4):
        rs = ReducedSystem(H, B, mu, ent, fr)
        d = rs.exact_step()
        ref = o.damped_solve(x, mu, res_mode=ol.RES_F32)
        assert _rel(d, ref) < 1e-9, (name, kw, mu, _rel(d, ref))
        # the certificate quantities of the exact step: a zero residual, r^T D^-1 r = 0; b^T A^-1 b is delta_s . b
        ds_, _ = rs.split(d)
        if len(ent):
            assert rs.rel_residual(ds_) < 1e-12
            rDr, bDb, bAb = rs.energy_norms(ds_)
            assert rDr < 1e-20 * bDb and abs(bAb - ds_ @ rs.b) <= 1e-10 * bAb
        if len(fr) and len(ent):
            # the fp32 operator: the same system to fp32 rounding of W
            rs32 = ReducedSystem(H, B, mu, ent, fr, w32=True)
            assert np.array_equal(rs32.A64, rs.A64) and not np.array_equal(rs32.A32, rs32.A64)
            assert rs32.rel_residual(ds_) < 1e-5 and rs32.rel_residual(ds_) > 0


def test_fixed_entities_are_identity_rows_with_a_zero_right_hand_side():
    ds, _ = load_golden("g1_cfg3_cut")
    o = ol.Oracle(ds)
    H, B = o.normal_equations(ds.x_full, res_mode=ol.RES_F32)
    fc = [c for c in range(ds.num_cams) if c != ds.root_cam][:2]
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker][1:4]
    held = held_mask(ds, len(B), fc + [ds.root_cam], fm)
    assert held.sum() == 6 * (len(fc) + len(fm))
    ent, fr = split_indices(ds)
    mu = float(np.diag(H).max()) * 1e-3
    d = ReducedSystem(H, B, mu, ent, fr, held=held).exact_step()
    assert np.all(d[held] == 0.0)
    keep = ~held
    ref = np.linalg.solve(H[np.ix_(keep, keep)] + mu * np.eye(keep.sum()), B[keep])
    assert _rel(d[keep], ref) < 1e-9, _rel(d[keep], ref)


def test_prior_blocks_join_after_the_damping():
    from reduced_system import prior_terms, slot_col
    ds, _ = load_golden("g1_cfg2")
    o = ol.Oracle(ds)
    x = ds.x_full
    H, B = o.normal_equations(x, res_mode=ol.RES_F32)
    rng = np.random.default_rng(3)
    priors = []
    for c in range(ds.num_cams):
        if c != ds.root_cam:
            col = slot_col(ds, "camera", c)
            A = rng.standard_normal((6, 6))
            priors.append(("camera", c, x[col:col + 6] + 0.01 * rng.standard_normal(6), 1e3 * (A @ A.T + 6 * np.eye(6))))
    Hp, Bp, _ = prior_terms(ds, x, priors, len(B))
    ent, fr = split_indices(ds)
    mu = float(np.diag(H).max()) * 1e-2
    d = ReducedSystem(H, B, mu, ent, fr, Hp=Hp, Bp=Bp).exact_step()
    ref = np.linalg.solve(H + mu * np.eye(len(B)) + Hp, B + Bp)
    assert _rel(d, ref) < 1e-9


def test_block_jacobi_follows_the_padded_entity_layout():
    # the 6-chunks of the entity unknowns, the intrinsics' 9 per camera included (C odd would leave a last chunk 3 wide)
    ds, _ = load_golden("g1_cfg2_intr")
    o = ol.Oracle(ds, intrinsics=True)
    x = _x0(ds, True)
    H, B = o.normal_equations(x, res_mode=ol.RES_F32)
    ent, fr = split_indices(ds, intrinsics=True)
    rs = ReducedSystem(H, B, float(np.diag(H).max()) * 1e-3, ent, fr)
    Dinv = rs.block_jacobi()
    n = len(ent)
    for o_ in range(0, n, 6):
        s = slice(o_, min(o_ + 6, n))
        np.testing.assert_allclose(Dinv[s, s] @ rs.A[s, s], np.eye(s.stop - s.start), atol=1e-9)
    off = Dinv.copy()
    for o_ in range(0, n, 6):
        off[o_:o_ + 6, o_:o_ + 6] = 0.0
    assert not off.any()
