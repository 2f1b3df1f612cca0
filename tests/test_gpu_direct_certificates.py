"""Certificates of the direct chain -- k_frame_inv -> k_schur / k_schur_mfma / k_schur<0,1> + k_schur_reduce -> k_ldl_* -> k_backsub -- in every launch
shape, against a float64 restatement of the damped reduced system built from the DEVICE'S OWN dense normal equations (tests/direct_certificate.py:
the observation passes are out of the comparison; what is left is frame inverse + Schur complement + LDL^T + both substitutions + frame
back-substitution).  Needs a real MI355X.

Every problem is created with solver="direct"; every step is taken at mu = 1e-3 max diag H and mu = max diag H unless stated; every test asserts
its premise (from the data set, solver_stats() or the launch counts of aar_get_kernel_times) before it certifies.  The tuning switches are read
when the problem is created (ba_capi.hip, "tuning switches of this problem"), so monkeypatch.setenv before Problem(...) selects the launch shape.
A data set's float64 system is built once, from the first problem that asks for it: problems of other launch shapes on the same set are certified
against that H -- theirs differs in summation order only, which is inside E_A.

Steps of a run: the take-back of the Schur complement (launch_schur with sign -1) is NOT on the path of a rejected try -- damped_try marks S as
eliminated (blocks_valid = false) and a rejected step's blocks are rebuilt from the observations before the re-damped Schur complement and
factorisation.  The take-back runs in damped_try (ba_capi.hip, "the speculative Schur complement was taken with another damping") on the first try
after a step that was ACCEPTED with gain < 0.94, whose speculative complement used mu / 3.  test_steps_of_a_run_with_rejected_tries certifies
both kinds: accepted steps with tries > 1, and steps that follow an accepted step with gain < 0.94.  Both are repairs of the speculative path; a
correctly predicted step -- no k_frame_inv, no Schur launch of its own, pass A's inverses and panels -- is certified in
tests/test_gpu_speculative_path.py.

Ratios: every certified step's |r| / bar and worst frame ratio are collected per family and printed when the module finishes (run with -s):
steps, worst, median.  The float64 reference's ratios on the same data sets are in tests/test_direct_certificate_host.py (worst 1.1e-3, medians
2e-5 .. 3e-4); NO DEVICE RATIO HAS BEEN MEASURED YET -- this module has not run on an MI355X, none of its families.
"""
import numpy as np
import pytest

import aar
import direct_cases as dc
import oracle_lib as ol
from conftest import load_golden
from direct_cases import ldl_env as _ldl_env, ldl_expected as _ldl_expected, run_ranks as _run_ranks
from direct_certificate import build_system, certify_direct, entity_blocks
from direct_run_certificate import mu_used as _mu_used
from reduced_system import slot_col

pytestmark = pytest.mark.gpu

MUS = (1e-3, 1.0)          # times max diag H
RATIOS = {}                # family -> [(|r| / bar, frame ratio)]
_SYS = {}                  # data-set key -> (blocks, max diag H, {mu factor: ReducedSystem})


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_report():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")
    yield
    print("\ndirect-chain certificate ratios (family: steps, worst, median |r| / bar; worst frame ratio)")
    for fam, v in sorted(RATIOS.items()):
        a = np.array(v)
        print("  %-18s %4d  %.3e  %.3e   %.3e" % (fam, len(a), a[:, 0].max(), np.median(a[:, 0]), a[:, 1].max()))


def _x0(p, ds, intr):
    return p.x_with_intrinsics(ds.x_full) if intr else np.asarray(ds.x_full, dtype=np.float64)


def _systems(key, p, ds, x, mus, opt, intr, fixed):
    if key not in _SYS:
        H, B, _ = p.eval_normal_equations(x)
        md = float(np.diag(H).max())
        _SYS[key] = (entity_blocks(ds, opt, intr), md, {m: build_system(ds, H, B, m * md, opt, intr, **fixed) for m in mus})
    return _SYS[key]


def _certify(family, key, p, ds, mus=MUS, opt=(True, True, True), intr=False, fixed=None, what=""):
    """certify the one-off steps of problem p at its start point; returns the steps"""
    assert p.solver_stats()["solver"] == "direct"
    x = _x0(p, ds, intr)
    blocks, md, sysm = _systems(key, p, ds, x, mus, opt, intr, fixed or {})
    z0 = p.extract_z(x)
    steps = []
    for m in mus:
        d = p.eval_damped_step(x, m * md)
        out = certify_direct(sysm[m], d, z0 + d, blocks, "%s %s %s mu %.3g" % (family, key, what, m * md))
        RATIOS.setdefault(family, []).append((out["ratio"], out["frame_ratio"]))
        steps.append(d)
    return steps


def _problem(ds, **kw):
    return aar.Problem(ds, solver="direct", **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# tile sweep: nT = 1 .. 14, both Schur kernels
@pytest.mark.parametrize("mfma", ["0", "1"])
@pytest.mark.parametrize("nT", list(range(1, 15)))
def test_tile_sweep(nT, mfma, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", mfma)
    ds = dc.sweep_ds(nT)
    assert 96 * dc.tiles_of(ds) == 96 * nT and 6 * (ds.num_cams + ds.num_markers) == 96 * nT - 18      # n_pad = 96 nT, the last tile 13/16 full
    with _problem(ds) as p:
        _certify("sweep mfma=" + mfma, "sweep%d" % nT, p, ds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# LDL^T launch structures
def _launch_counts(p, ds, mu):
    p.set_kernel_profiling(True)
    p.eval_damped_step(np.asarray(ds.x_full, dtype=np.float64), mu)
    kt = p.kernel_times()
    p.set_kernel_profiling(False)
    return {k: v[1] for k, v in kt.items()}


@pytest.mark.parametrize("lookahead", [0, 1])
@pytest.mark.parametrize("fused", [0, 2, 3, 5])
@pytest.mark.parametrize("nT", [2, 3, 4, 5, 8, 14])
def test_ldl_launch_structures(nT, fused, lookahead, monkeypatch):
    _ldl_env(monkeypatch, fused, lookahead)
    ds = dc.sweep_ds(nT)
    with _problem(ds) as p:
        _certify("ldl structures", "sweep%d" % nT, p, ds, what="fused %d lookahead %d" % (fused, lookahead))
        if (fused, lookahead) in ((2, 1), (0, 0)):
            # premise: the intended kernels ran
            cnt = _launch_counts(p, ds, _SYS["sweep%d" % nT][1])
            want = _ldl_expected(nT, fused, lookahead, 1)
            k = cnt["k_ldl_diag"] // nT
            assert k >= 1 and {n: cnt[n] for n in want} == {n: k * v for n, v in want.items()}, (cnt, want)


@pytest.mark.parametrize("nT", [2, 3, 4, 5, 8, 14])
def test_ldl_back_substitution_as_its_own_launch(nT, monkeypatch):
    _ldl_env(monkeypatch, bs_rides=0)
    ds = dc.sweep_ds(nT)
    with _problem(ds) as p:
        _certify("ldl structures", "sweep%d" % nT, p, ds, what="AAR_BS_RIDES=0")
        cnt = _launch_counts(p, ds, _SYS["sweep%d" % nT][1])
        assert cnt["k_ldl_backsolve"] == cnt["k_ldl_diag"] // nT >= 1, cnt


# ---------------------------------------------------------------------------------------------------------------------------------------------
# gauge and fixed rows at tile boundaries
@pytest.mark.parametrize("cams,row", [(16, 96), (15, 90), (34, 204)])
def test_root_marker_rows_at_tile_boundaries(cams, row):
    ds = dc.gauge_ds(cams, 3)
    assert dc.tiles_of(ds) == 3 and 6 * (ds.num_cams + ds.root_marker) == row      # first rows of tile 1 / last rows of tile 0 / inside tile 2
    with _problem(ds) as p:
        _certify("gauge rows", "gauge_c%d" % cams, p, ds)


def _fixed(ds):
    fc = [c for c in range(ds.num_cams) if c != ds.root_cam][:2]
    fm = [m for m in range(ds.num_markers) if m != ds.root_marker][3:4]
    return dict(fixed_cams=fc, fixed_markers=fm)


@pytest.mark.parametrize("which", ["cams_off", "markers_off", "fixed"])
@pytest.mark.parametrize("tiles", [3, 5])
def test_identity_tiles_and_caller_fixed_entities(tiles, which):
    ds = dc.gauge_ds(16, tiles)
    assert dc.tiles_of(ds) == tiles and ds.num_cams == 16      # cameras off: the whole of tile 0 is identity; markers off: every tile behind it
    opt = dict(cams_off=(False, True, True), markers_off=(True, False, True), fixed=(True, True, True))[which]
    fx = _fixed(ds) if which == "fixed" else {}
    with _problem(ds, optimize=opt, **fx) as p:
        steps = _certify("gauge rows", "%s_%d" % (which, tiles), p, ds, opt=opt, fixed=fx)
        if fx:
            for d in steps:
                for c in fx["fixed_cams"]:
                    assert np.all(d[slot_col(ds, "camera", c):slot_col(ds, "camera", c) + 6] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Schur work lists of the output-stationary kernel
def _pairs_per_entity(ds):
    of, oc, om = np.asarray(ds.obs_frame), np.asarray(ds.obs_cam), np.asarray(ds.obs_marker)
    return [len(set(of[oc == c])) for c in range(ds.num_cams)] + [len(set(of[om == m])) for m in range(ds.num_markers)]


@pytest.mark.parametrize("knob,value", [("AAR_SCHUR_ITEM", 4), ("AAR_SCHUR_ITEM", 8), ("AAR_SCHUR_ITEM", 100000),
                                        ("AAR_SCHUR_WINDOW", 1), ("AAR_SCHUR_WINDOW", 7), ("AAR_SCHUR_WINDOW", 64)])
@pytest.mark.parametrize("det", [False, True])
def test_schur_work_lists_cut_by_pair_count_and_by_frame_window(knob, value, det, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", "0")
    monkeypatch.setenv(knob, str(value))
    ds = dc.worklist_ds(60)
    ppe = _pairs_per_entity(ds)
    assert dc.tiles_of(ds) == 2 and ds.num_frames == 60
    if knob == "AAR_SCHUR_ITEM":
        assert (max(ppe) > 4 * value) if value < 100 else (max(ppe) < value), ppe       # several items per entity / one
    else:
        assert (60 > 4 * value) if value < 64 else (60 < value)                          # several windows / one
    with _problem(ds, deterministic=det) as p:
        assert p.solver_stats()["deterministic"] == det
        _certify("work lists" + (" det" if det else ""), "worklist_F60", p, ds, what="%s=%d" % (knob, value))


@pytest.mark.parametrize("F", [3, 8, 9, 60])
@pytest.mark.parametrize("det", [False, True])
def test_schur_work_list_in_xcd_order(F, det, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", "0")
    monkeypatch.setenv("AAR_SCHUR_XCD", "1")
    ds = dc.worklist_ds(F)
    assert ds.num_frames == F and min(dc.frame_entity_counts(ds)) > 0      # F < 8: some of the eight frame ranges are empty -- padded items
    with _problem(ds, deterministic=det) as p:
        _certify("work lists" + (" det" if det else ""), "worklist_F%d" % F, p, ds, what="AAR_SCHUR_XCD=1")


@pytest.mark.parametrize("env", [{}, {"AAR_SCHUR_XCD": "1"}, {"AAR_SCHUR_WINDOW": "7"}, {"AAR_SCHUR_MFMA": "1"}])
def test_a_marker_seen_nowhere_and_one_seen_once(env, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ds = dc.without_pairs(dc.worklist_ds(60), 7, 11)
    ppe = _pairs_per_entity(ds)
    assert ppe[ds.num_cams + 7] == 0 and ppe[ds.num_cams + 11] == 1
    with _problem(ds) as p:
        steps = _certify("work lists", "worklist_unseen", p, ds, what=str(env))
        for d in steps:      # the unseen marker's step is exactly zero: its rows hold the damping and a zero right-hand side
            assert np.all(d[slot_col(ds, "marker", 7):slot_col(ds, "marker", 7) + 6] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# k_schur<3>: frames of more than 64 entities under the output-stationary kernel
@pytest.mark.parametrize("markers", [84, 92])
def test_wide_frames_take_the_prefetching_schur_kernel(markers, monkeypatch):
    ds = dc.wide_frames_ds(markers)
    kf = dc.frame_entity_counts(ds)
    A = ds.num_cams + ds.num_markers
    assert max(kf) > 64 and min(kf) < 30 and any(30 < k < 60 for k in kf) and any(60 < k <= 64 for k in kf), kf      # (slots: both sides of 30 and of 60)
    if markers == 84:
        assert A < 96                         # the output-stationary kernel is the default below 96 entities
        monkeypatch.delenv("AAR_SCHUR_MFMA", raising=False)
    else:
        assert A >= 96
        monkeypatch.setenv("AAR_SCHUR_MFMA", "0")
    with _problem(ds) as p:
        _certify("k_schur<3>", "wide_%d" % markers, p, ds)
        cnt = _launch_counts(p, ds, _SYS["wide_%d" % markers][1])
        assert cnt["k_schur"] >= 1, cnt


# ---------------------------------------------------------------------------------------------------------------------------------------------
# k_schur_mfma
@pytest.mark.parametrize("split", [1, 3, 12, 100000])
def test_mfma_schur_frame_pieces(split, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", "1")
    monkeypatch.setenv("AAR_SCHUR_SPLIT", str(split))
    ds = dc.worklist_ds(60)
    with _problem(ds) as p:
        _certify("k_schur_mfma", "worklist_F60", p, ds, what="AAR_SCHUR_SPLIT=%d" % split)


@pytest.mark.parametrize("passa", ["0", "1"])
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 8, 9])
def test_mfma_schur_short_frame_lists(F, passa, monkeypatch):
    # (these one-off steps do NOT read pass A's panels: eval_damped_step asks pass A for no predicted damping, so the panels come from k_schur_fill
    #  and the inverses from k_frame_inv whatever AAR_DENSE_FROM_PASSA says -- both parameter values run the same code here.  Where the switch
    #  selects code, inside an LM run, it is certified by tests/test_gpu_speculative_path.py)
    monkeypatch.setenv("AAR_SCHUR_MFMA", "1")
    monkeypatch.setenv("AAR_DENSE_FROM_PASSA", passa)
    ds = dc.mfma_frames_ds(F)
    assert ds.num_frames == F and dc.tiles_of(ds) == 2 and min(dc.frame_entity_counts(ds)) > 0
    with _problem(ds) as p:
        _certify("k_schur_mfma", "mfma_F%d" % F, p, ds, what="AAR_DENSE_FROM_PASSA=" + passa)


@pytest.mark.parametrize("dense", [31, 32, 33])
def test_mfma_schur_dense_count_at_the_padding_boundary(dense, monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_MFMA", "1")
    ds = dc.dense_count_ds(dense - 1)
    assert dc.seen_entities(ds) + 1 == dense          # Ad = 32, 32, 64
    with _problem(ds) as p:
        _certify("k_schur_mfma", "dense_%d" % dense, p, ds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# deterministic mode: k_schur<0, 1> + k_schur_reduce
@pytest.mark.parametrize("nT", [1, 3, 7])
def test_deterministic_tile_sweep_and_equal_bits(nT):
    ds = dc.sweep_ds(nT)
    steps = []
    for _ in range(2):
        with _problem(ds, deterministic=True) as p:
            assert p.solver_stats()["deterministic"]
            steps.append(_certify("deterministic", "sweep%d" % nT, p, ds))
    for a, b in zip(*steps):
        assert np.array_equal(a, b)


def test_deterministic_work_list_equal_bits(monkeypatch):
    monkeypatch.setenv("AAR_SCHUR_XCD", "1")
    ds = dc.worklist_ds(3)
    steps = []
    for _ in range(2):
        with _problem(ds, deterministic=True) as p:
            steps.append(_certify("deterministic", "worklist_F3", p, ds, what="AAR_SCHUR_XCD=1"))
    for a, b in zip(*steps):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# features
def _priors(ds, x):
    rng = np.random.default_rng(3)
    pr = []
    for c in range(ds.num_cams):
        if c != ds.root_cam:
            col = slot_col(ds, "camera", c)
            A = rng.standard_normal((6, 6))
            pr.append(("camera", c, x[col:col + 6] + np.r_[0.02 * rng.standard_normal(3), 0.01 * rng.standard_normal(3)], 1e3 * (A @ A.T + 6 * np.eye(6))))
    return pr


@pytest.mark.parametrize("feature", ["huber", "intrinsics", "priors"])
def test_features(feature):
    ds, _ = load_golden(dict(huber="g1_cfg2_huber", intrinsics="g1_cfg2_intr", priors="g1_cfg3_cut")[feature])
    kw = dict(huber=dict(with_huber=True), intrinsics=dict(intrinsics=True), priors=dict(priors=_priors(ds, np.asarray(ds.x_full))))[feature]
    with _problem(ds, **kw) as p:
        _certify("features", feature, p, ds, intr=feature == "intrinsics")       # (the device's H carries the Huber weights and the priors' blocks)


@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("world,nT", [(2, 2), (3, 5)])
def test_sharded_system_as_it_lies_and_packed(world, nT, pack, monkeypatch):
    monkeypatch.setenv("AAR_PACK_SYSTEM", pack)
    ds = dc.sweep_ds(nT)
    key = "sweep%d" % nT
    x = np.asarray(ds.x_full, dtype=np.float64)
    with _problem(ds) as p:      # the ONE-rank device H of the same problem: the ranks' sum differs from it in summation order only
        blocks, md, sysm = _systems(key, p, ds, x, MUS, (True, True, True), False, {})
        z0 = p.extract_z(x)

    def solve(comm, rank):
        with aar.Problem(ds, comm=comm, solver="direct") as q:
            return [q.eval_damped_step(x, m * md) for m in MUS], q.local_obs
    res = _run_ranks(world, solve)
    assert all(r[1] > 0 for r in res), [r[1] for r in res]
    for i, m in enumerate(MUS):
        for r in range(world):      # (every rank returns the whole gathered step)
            d = res[r][0][i]
            out = certify_direct(sysm[m], d, z0 + d, blocks, "world %d rank %d nT %d AAR_PACK_SYSTEM=%s mu %.3g" % (world, r, nT, pack, m * md))
            RATIOS.setdefault("sharded", []).append((out["ratio"], out["frame_ratio"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# steps of a run with rejected tries
def test_steps_of_a_run_with_rejected_tries():
    ds = aar.synth(2, num_frames=40, init_scale=20.0)
    o = ol.Oracle(ds)
    x0 = np.asarray(ds.x_full, dtype=np.float64)
    with _problem(ds) as p:
        zs = [p.extract_z(x0)]
        p.set_step_callback(lambda z: zs.append(z))
        _, rep = p.lm_solve(x0, params=aar.lm_default_params(tau=1e-6))
        p.set_step_callback(None)
        trace = rep["trace"]
        assert any(t["tries"] > 1 for t in trace), [t["tries"] for t in trace]
        H0, _, _ = p.eval_normal_equations(x0)
        mu0 = 1e-6 * float(np.diag(H0).max())
        ok = [k for k, t in enumerate(trace) if t["accepted"] and k + 1 < len(zs) and all(u["accepted"] for u in trace[:k])]
        redamped = [k for k in ok if trace[k]["tries"] > 1][:3]
        taken_back = [k for k in ok if k > 0 and trace[k - 1]["gain"] < 0.94 and trace[k]["tries"] == 1][:3]
        assert redamped and taken_back, (redamped, taken_back)
        blocks = entity_blocks(ds)
        for k in sorted(set(redamped + taken_back)):
            mu = _mu_used(trace, k, mu0)
            H, B, _ = p.eval_normal_equations(o.merge_z(x0, zs[k]))
            rs = build_system(ds, H, B, mu)
            out = certify_direct(rs, zs[k + 1] - zs[k], zs[k + 1], blocks, "LM step %d (mu %.3g, %d tries, gain before %.3g)"
                                 % (k, mu, trace[k]["tries"], trace[k - 1]["gain"] if k else 0.0))
            RATIOS.setdefault("steps of a run", []).append((out["ratio"], out["frame_ratio"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# full size: config 3 whole (276 reduced unknowns, 500 frames), config 5 as a slice of its shape (16 cameras / 200 markers, 40 frames), one damping each
@pytest.mark.parametrize("shape", ["cfg3", "cfg5_shaped"])
def test_full_size(shape):
    ds = aar.synth(3) if shape == "cfg3" else aar.synth(5, num_frames=40)
    with _problem(ds) as p:
        _certify("full size", shape, p, ds, mus=(1e-3,))
