"""The smoothed track at any time (aar_track_smooth_query): pose and covariance block at query times between, on and
outside the frame times.  Needs a real MI355X.

The answer at a time t is what the smoother reports for a frame without detections inserted at t, so both yardsticks are existing device code
on the AUGMENTED data set (tests/smooth_query_cases.inserted):
  1. numpy.linalg.inv of the dense H' built from aar_track_smooth_system's blocks of the augmented data set; bar 10 eps kappa_2(H'), Frobenius
     error of the queried block over the Frobenius norm of the yardstick's block (the forward-error order of an inverse, section 28's bar);
  2. the same block from aar_track_smooth_covariance on the augmented data set; bar 20 eps kappa_2(H') (both sides owe 10 to the inverse).
Poses: smooth_restated.geodesic within 1e-12 (the bar section 16 uses for quantities that measure a few 1e-15), as rotation vectors and as
rotation matrices; the shapes stay below 3 rad (the restated logarithm is not written for angles near pi).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aar
import smooth_cases as sc
import smooth_query_cases as sqc
import smooth_query_restated as sqr
import smooth_restated as sr
import track_restated as tr
from conftest import PKG, ROOT
from test_gpu_track_smooth import SROT, STRANS, _gaps, _golden_track, _problem, _shape_dataset

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")


def _kappa(H):
    ev = np.linalg.eigvalsh(H)
    assert ev[0] > 0
    return float(ev[-1] / ev[0])


def _frame_time(F):
    """non-uniform times at 2, 5 and 65 frames; none at 1 and 3: the library's own 0, 1, 2, ..."""
    return 0.25 + _gaps(F) if F in (2, 5, 65) else None


def _gaps_of(F):
    """the gaps queried: the first and the last, and at 65 frames (sc.emptied: 0, 21 .. 30, 64) one beside an emptied frame with an observed one on
    its other side, one between two emptied frames, one between two observed frames"""
    if F < 2:
        return []
    return sorted({0, F - 2} | ({20, 25, 40} if F == 65 else set()))


def _query_times(gaps, times):
    out = []
    for g in gaps:
        for al in (1e-3, 0.5):
            out.append(times[g] + al * (times[g + 1] - times[g]))
    return out + [times[0] - 0.3, times[-1] + 4.0]


def _rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


_CASES = {}


def _case(F, delta=None, ds=None):
    """the query call of one shape (a given data set: uniform times, three gaps) and, per query, the two yardsticks from the augmented data set
    -- computed once, shared, not modified"""
    key = (F, delta, ds is None)
    if key in _CASES:
        return _CASES[key]
    if ds is None:
        ds = _shape_dataset(F)
        x0, ft, gaps = sc.track_start(ds), _frame_time(F), _gaps_of(F)
    else:
        x0, ft, gaps = np.array(ds.x_full), None, [0, F // 3, F // 2]
    assert ds.num_frames == F
    times = sqr.times_of(F, ft)
    qt = np.array(_query_times(gaps, times))
    with _problem(ds, delta) as p:
        pose, cov, seg, rep = p.track_smooth_query(x0, SROT, STRANS, qt, frame_time=ft)
        pose_only, none, seg_only, rep_only = p.track_smooth_query(x0, SROT, STRANS, qt, frame_time=ft, covariance=False)
        S, R, crep = p.track_smooth_covariance(x0, SROT, STRANS, frame_time=ft)
    assert none is None
    dense, parent, kappa, zin = [], [], [], []
    for t in qt:
        ds2, x2, ft2, pos = sqc.inserted(ds, x0, ft, t)
        with _problem(ds2, delta) as p:
            gd, go, _, _, _ = p.track_smooth_system(x2, SROT, STRANS, 0.0, frame_time=ft2)
            S2, _, _ = p.track_smooth_covariance(x2, SROT, STRANS, frame_time=ft2)
        H2 = sr.dense(gd, go)
        dense.append(np.linalg.inv(H2)[6 * pos:6 * pos + 6, 6 * pos:6 * pos + 6])
        parent.append(S2[pos])
        kappa.append(_kappa(H2))
        zin.append(sqc.frames_of(ds2, x2)[pos])
    out = dict(ds=ds, x0=x0, ft=ft, times=times, qt=qt, pose=pose, cov=cov, seg=seg, rep=rep, pose_only=pose_only, seg_only=seg_only,
               rep_only=rep_only, S=S, R=R, crep=crep, dense=dense, parent=parent, kappa=kappa, zin=zin)
    _CASES[key] = out
    return out


# ---- 1. covariance against the dense inverse of the augmented system ----
@pytest.mark.parametrize("F", [1, 2, 3, 5, 65])
def test_covariance_against_the_dense_inverse(F):
    c = _case(F)
    worst = 0.0
    for k, t in enumerate(c["qt"]):
        e = _rel(c["cov"][k], c["dense"][k])
        worst = max(worst, e / (EPS * c["kappa"][k]))
        print("F %d t %.6g (segment %d): kappa %.3e, block %.2e = %.4f eps kappa" % (F, t, c["seg"][k], c["kappa"][k], e, e / (EPS * c["kappa"][k])))
        assert e <= 10 * EPS * c["kappa"][k], (t, e, 10 * EPS * c["kappa"][k])
    print("F %d: largest %.4f eps kappa_2(H')" % (F, worst))
    assert np.all(np.isfinite(c["cov"])) and min(np.linalg.eigvalsh(m)[0] for m in c["cov"]) > 0
    n_in = 2 * len(_gaps_of(F))
    rep = c["rep"]
    assert (rep["num_queries"], rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (n_in + 2, n_in, 0, 2)
    assert rep["launches"] == c["crep"]["launches"] + 1
    for k in ("num_residuals", "num_vars", "data_cost", "prior_cost", "sigma2"):
        assert rep[k] == c["crep"][k], k


# ---- 2. against the parent commit's code on the augmented data set ----
@pytest.mark.parametrize("F", [1, 2, 3, 5, 65])
def test_covariance_against_the_covariance_of_the_augmented_set(F):
    c = _case(F)
    for k, t in enumerate(c["qt"]):
        e = _rel(c["cov"][k], c["parent"][k])
        print("F %d t %.6g: against aar_track_smooth_covariance %.2e = %.4f eps kappa" % (F, t, e, e / (EPS * c["kappa"][k])))
        assert e <= 20 * EPS * c["kappa"][k], (t, e)


# ---- 3. pose ----
@pytest.mark.parametrize("F", [1, 2, 3, 5, 65])
def test_pose(F):
    c = _case(F)
    z = sqc.frames_of(c["ds"], c["x0"])
    for k, t in enumerate(c["qt"]):
        a, kind = sqr.locate(c["times"], t)
        assert c["seg"][k] == a
        if kind == "inside":
            want = sr.geodesic(z[a], z[a + 1], (t - c["times"][a]) / (c["times"][a + 1] - c["times"][a]))
            assert np.array_equal(want, c["zin"][k])
            assert np.abs(tr.rodrigues(c["pose"][k][:3]) - tr.rodrigues(want[:3])).max() <= 1e-12
            assert np.abs(c["pose"][k][3:] - want[3:]).max() <= 1e-12
            assert np.linalg.norm(want[:3]) < 3.0 and np.abs(c["pose"][k] - want).max() <= 1e-12, (t, c["pose"][k], want)
            assert np.linalg.norm(c["pose"][k][:3]) <= np.pi + 1e-12
        else:
            assert np.array_equal(c["pose"][k], z[0] if kind == "before" else z[F - 1])      # the end pose, bit for bit
    assert np.array_equal(c["pose_only"], c["pose"]) and np.array_equal(c["seg_only"], c["seg"])
    assert c["rep_only"]["launches"] == 1 and c["rep_only"]["sigma2"] == 0.0 and c["rep_only"]["num_outside"] == 2


# ---- 4. on a frame time ----
@pytest.mark.parametrize("F", [1, 3, 65])
def test_on_a_frame_time(F):
    c = _case(F)
    z = sqc.frames_of(c["ds"], c["x0"])
    with aar.Problem(c["ds"]) as p:
        pose, cov, seg, rep = p.track_smooth_query(c["x0"], SROT, STRANS, c["times"], frame_time=c["ft"])
    assert np.array_equal(pose, z) and np.array_equal(cov, c["S"]) and np.array_equal(seg, np.arange(F))
    assert (rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (0, F, 0)


# ---- 5. shapes and bits ----
def _mixed_times(times, Q, seed):
    """Q query times: inside, on frames, outside, with duplicates, shuffled"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(times[0] - 2.0, times[-1] + 2.0, size=Q)
    t[::5] = rng.choice(times, size=len(t[::5]))              # on frame times
    if Q >= 8:
        t[3::7] = t[1]                                        # duplicates
    rng.shuffle(t)
    return t


@pytest.mark.parametrize("Q", [0, 1, 64, 65, 257])
def test_shapes_and_bits(Q):
    c = _case(65)
    ds, x0, ft, times = c["ds"], c["x0"], c["ft"], c["times"]
    qt = _mixed_times(times, Q, 5 + Q)
    keep = np.array(x0)
    with aar.Problem(ds) as p:
        a0 = p.track_smooth(x0, SROT, STRANS, frame_time=ft)
        pose, cov, seg, rep = p.track_smooth_query(x0, SROT, STRANS, qt, frame_time=ft)
        pose2, cov2, seg2, rep2 = p.track_smooth_query(x0, SROT, STRANS, qt, frame_time=ft)
        a1 = p.track_smooth(x0, SROT, STRANS, frame_time=ft)
        alone = {}
        for t in np.unique(qt):
            alone[t] = p.track_smooth_query(x0, SROT, STRANS, [t], frame_time=ft)
    assert np.array_equal(x0, keep)
    assert pose.shape == (Q, 6) and cov.shape == (Q, 6, 6) and seg.shape == (Q,)
    assert np.array_equal(pose, pose2) and np.array_equal(cov, cov2) and np.array_equal(seg, seg2)       # two calls: identical
    for u, v in zip(a0, a1):                                                                             # no state is left behind
        if isinstance(u, dict):
            assert all(k == "seconds" or u[k] == v[k] for k in u)
        else:
            assert np.array_equal(u, v)
    kinds = [sqr.locate(times, t) for t in qt]
    for k, t in enumerate(qt):
        p1, c1, s1, _ = alone[t]
        assert pose[k].tobytes() == p1[0].tobytes() and cov[k].tobytes() == c1[0].tobytes() and seg[k] == s1[0] == kinds[k][0], (k, t)
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))                                                   # symmetric to the bit
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(pose))
    count = [sum(kd == w for _, kd in kinds) for w in ("inside", "on")]
    assert (rep["num_queries"], rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (Q, count[0], count[1], Q - sum(count))
    if Q >= 64:
        assert min(count) > 0 and Q - sum(count) > 0
    assert rep["launches"] == (c["crep"]["launches"] + 1 if Q else 0)
    if Q:
        # the covariance grows into a gap and beyond the ends: an inserted frame is less certain than an observed neighbour
        tvar = np.einsum("qii->q", cov[:, 3:, 3:])
        k = int(np.argmax(qt))
        assert kinds[k][1] != "after" or tvar[k] > np.trace(c["S"][64][3:, 3:])


# ---- 6. refusals ----
def _last_error():
    return aar.lib().aar_last_error().decode("utf-8", "replace")


def _raw(p, x0, qt, sp=None, pose=True, cov=True, seg=True, report=True, struct_size=None, fill=7.0):
    x = np.array(p._x(x0), dtype=np.float64)
    keep = x.copy()
    spar = aar.SmoothParams(SROT, STRANS) if sp is None else sp
    qt = np.ascontiguousarray(qt, dtype=np.float64)
    Q = len(qt)
    po, co, sg = np.full((max(Q, 1), 6), fill), np.full((max(Q, 1), 36), fill), np.full(max(Q, 1), 77, dtype=np.int32)
    rep = aar.CSmoothQueryReport()
    C.memset(C.byref(rep), 0x55, C.sizeof(rep))
    rep.struct_size = C.sizeof(rep) if struct_size is None else struct_size
    code = aar.lib().aar_track_smooth_query(p.handle, aar._dptr(x), C.byref(spar.c), Q, aar._dptr(qt), aar._dptr(po) if pose else None,
                                            aar._dptr(co) if cov else None, sg.ctypes.data_as(C.POINTER(C.c_int32)) if seg else None,
                                            C.byref(rep) if report else None)
    assert np.array_equal(x, keep)
    return code, po, co, sg, rep


def test_refusals():
    c = _case(5)
    ds, x0 = c["ds"], c["x0"]
    with aar.Problem(ds) as p:
        rel = aar.SmoothParams(SROT, STRANS, None, np.zeros((4, 6)))
        code, po, co, sg, _ = _raw(p, x0, [0.5], sp=rel)
        assert code == aar.AAR_ERR_UNSUPPORTED and "rel_motion" in _last_error() and np.all(po == 7.0) and np.all(co == 7.0) and np.all(sg == 77)
        code, po, co, sg, _ = _raw(p, x0, [0.5, 1.5, 0.0, np.nan, 2.0])
        assert code == aar.AAR_ERR_INVALID and "query_time[3]" in _last_error() and np.all(po == 7.0) and np.all(co == 7.0)
        with pytest.raises(aar.AarError) as e:
            p.track_smooth_query(x0, -1.0, STRANS, [0.5])
        assert e.value.code == aar.AAR_ERR_INVALID and "sigma_rot" in str(e.value)
        # NULL outputs and a caller compiled against a shorter report
        code, po, co, sg, rep = _raw(p, x0, [0.5, 1.0, 9.0])
        assert code == 0 and not np.any(po == 7.0) and not np.any(co == 7.0) and list(sg) == [0, 1, 4]
        for kw in (dict(pose=False), dict(seg=False), dict(report=False), dict(pose=False, seg=False, report=False)):
            code, po2, co2, sg2, _ = _raw(p, x0, [0.5, 1.0, 9.0], **kw)
            assert code == 0 and np.array_equal(co2, co), kw
            assert np.array_equal(po2, po) if kw.get("pose", True) else np.all(po2 == 7.0)
            assert np.array_equal(sg2, sg) if kw.get("seg", True) else np.all(sg2 == 77)
        cut = aar.CSmoothQueryReport.num_queries.offset
        code, _, _, _, rep3 = _raw(p, x0, [0.5, 1.0, 9.0], struct_size=cut)
        assert code == 0 and rep3.struct_size == cut and rep3.sigma2 == rep.sigma2 and rep3.num_vars == 30
        assert bytes(bytearray(rep3)[cut:]) == b"\x55" * (C.sizeof(rep3) - cut)
    nothing = sc.without_frames(aar.synth(2, num_frames=6), range(6))                  # a recording without any detection
    assert nothing.num_obs == 0
    with aar.Problem(nothing) as p:
        code, po, co, sg, _ = _raw(p, sc.track_start(nothing), [0.5, 2.0, -1.0])
        assert code == aar.AAR_ERR_NUMERIC and np.all(po == 7.0) and np.all(co == 7.0) and np.all(sg == 77)
        code, po, co, sg, _ = _raw(p, sc.track_start(nothing), [0.5, 2.0, -1.0], cov=False)      # poses alone need no inverse
        assert code == 0 and not np.any(po == 7.0) and list(sg) == [0, 2, -1]


def test_unsupported_behind_a_communicator():
    ds, _ = _golden_track("g_track_cfg2")
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(ds, comm=comm) as p:
            with pytest.raises(aar.AarError) as e:
                p.track_smooth_query(ds.x_full, SROT, STRANS, [0.5])
            assert e.value.code == aar.AAR_ERR_UNSUPPORTED
    finally:
        comm.close()
        group.close()


# ---- 7. a Huber problem ----
def test_huber_problem():
    ds, _ = _golden_track("g_track_cfg2_huber")
    F = ds.num_frames
    assert F >= 3
    c = _case(F, 1.0, ds=ds)
    with aar.Problem(ds) as p:
        plain = p.track_smooth_query(ds.x_full, SROT, STRANS, c["qt"])[1]
    for k, t in enumerate(c["qt"]):
        e = _rel(c["cov"][k], c["dense"][k])
        print("huber t %.6g: kappa %.3e, block %.2e = %.4f eps kappa" % (t, c["kappa"][k], e, e / (EPS * c["kappa"][k])))
        assert e <= 10 * EPS * c["kappa"][k], (t, e)
    # the weights are in the blocks: down-weighted detections leave the poses less certain
    assert np.einsum("qii->", c["cov"]) > np.einsum("qii->", plain)


# ---- 8. the C++ mirror and the command-line driver ----
def _kv(stdout):
    return dict(l.split(" = ") for l in stdout.splitlines() if " = " in l)


def test_mapper_track_smooth_query(tmp_path):
    exe = str(tmp_path / "smooth_query_mapper_main")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "tools", "smooth_query_mapper_main.cpp"), "-o", exe, "-L" + PKG,
                         "-laar", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    ds = aar.synth(2)
    F = ds.num_frames
    ft = np.asarray(ds.frame_ids, dtype=np.float64)
    qt = np.array([ft[0] - 1.5, ft[0], ft[0] + 0.25, 0.5 * (ft[40] + ft[41]), ft[50], ft[-1] + 2.0])
    run = subprocess.run([exe, "2", repr(SROT), repr(STRANS)] + [repr(float(t)) for t in qt], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    kv = _kv(run.stdout)
    x0 = sc.track_start(ds)
    with aar.Problem(ds) as p:
        xt, _, _ = p.track(x0, aar.lm_default_params())
        xs, _, _, _ = p.track_smooth(xt, SROT, STRANS, frame_time=ft)
        pose, cov, seg, rep = p.track_smooth_query(xs, SROT, STRANS, qt, frame_time=ft)
    assert [int(kv[k]) for k in ("queries", "inside", "on_frame", "outside", "launches")] == \
        [rep[k] for k in ("num_queries", "num_inside", "num_on_frame", "num_outside", "launches")]
    assert (rep["num_inside"], rep["num_on_frame"], rep["num_outside"]) == (2, 2, 2)
    assert int(kv["pose_launches"]) == 1 and int(kv["same_poses"]) == 1 and int(kv["cov_without"]) == 0
    # (the mapper carries its poses as 4x4 matrices between its calls: 1e-8 in the poses as tests/test_gpu_track_smooth.py holds them; the blocks
    # follow the point)
    np.testing.assert_allclose(float(kv["sigma2"]), rep["sigma2"], rtol=1e-7)
    for k in range(len(qt)):
        assert int(kv["segment%d" % k]) == seg[k]
        pm = np.array([float(v) for v in kv["pose%d" % k].split()])
        cm = np.array([float(v) for v in kv["cov%d" % k].split()]).reshape(6, 6)
        assert np.abs(pm - pose[k]).max() <= 1e-8, k
        assert np.abs(cm - cov[k]).max() <= 1e-6 * np.abs(cov[k]).max(), k


def parse_resampled_yaml(path):
    """(sigma2, n, times [K], segments [K], poses [K, 6], scaled blocks [K, 6, 6]) of final.resampled.yaml"""
    txt = open(path).read()
    assert txt.startswith("%YAML:1.0\n---\nsigma2: ")
    sigma2 = float(re.search(r"^sigma2: (\S+)$", txt, re.M).group(1))
    n = int(re.search(r"^resample: (\d+)$", txt, re.M).group(1))
    rows = re.findall(r"- \{ time: (\S+), segment:(-?\d+), pose: \[([^\]]*)\],\s*covariance: !!opencv-matrix \{ rows:6, cols:6, dt:d, data:\[([^\]]*)\] \} \}", txt)
    t = np.array([float(r[0]) for r in rows])
    seg = np.array([int(r[1]) for r in rows])
    pose = np.array([[float(v) for v in r[2].split(",")] for r in rows])
    blk = np.array([[float(v) for v in r[3].split(",")] for r in rows]).reshape(-1, 6, 6)
    return sigma2, n, t, seg, pose, blk


def test_find_solution_resample_switch(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    assert subprocess.run([exe, "--synth", "2", folder], capture_output=True, text=True).returncode == 0
    # as tests/test_gpu_track_smooth_covariance.py: the recording is cut before config 2's frames that turn through pi, where the solution file's
    # rotation-vector round trip changes the coordinates of the blocks
    full = aar.solution_read(os.path.join(folder, "initial.solution"))
    FK = 90
    n0 = sc.ns(full)
    keep = np.asarray(full.obs_frame) < FK
    cut = sc.copy_of(full, num_frames=FK, frame_ids=full.frame_ids[:FK], obs_frame=full.obs_frame[keep], obs_cam=full.obs_cam[keep],
                     obs_marker=full.obs_marker[keep], obs_uv=full.obs_uv[keep], x_full=np.array(full.x_full[:n0 + 6 * FK]), x_truth=None)
    os.remove(os.path.join(folder, "initial.solution"))
    aar.solution_write(os.path.join(folder, "initial_tracking_only.solution"), cut)
    base = [exe, folder, "0.05", "x", "-from-initial", "-solver", "direct", "-tracking-only"]
    run = subprocess.run(base + ["-smooth", repr(SROT), repr(STRANS), "-resample", "2"], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, AAR_DETERMINISTIC="1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert len([l for l in run.stdout.splitlines() if l.startswith("resample: ")]) == 1 and "smooth: " in run.stdout, run.stdout
    sigma2, n, t, seg, pose, blk = parse_resampled_yaml(os.path.join(folder, "final.resampled.yaml"))
    got = aar.solution_read(os.path.join(folder, "final_tracking_only.solution"))
    F = got.num_frames
    ft = np.asarray(got.frame_ids, dtype=np.float64)
    z = got.x_full[n0:n0 + 6 * F].reshape(F, 6)
    assert F == FK and n == 2 and len(t) == 2 * F - 1 and np.linalg.norm(z[:, :3], axis=1).max() < 3.0
    mid = ft[:-1] + (ft[1:] - ft[:-1]) * 0.5
    assert np.array_equal(t[0::2], ft) and np.array_equal(t[1::2], mid)
    assert np.array_equal(seg[0::2], np.arange(F)) and np.array_equal(seg[1::2], np.arange(F - 1))
    with aar.Problem(got) as p:
        pm, cm, _, rep = p.track_smooth_query(got.x_full, SROT, STRANS, mid, frame_time=ft)
        S, _, _ = p.track_smooth_covariance(got.x_full, SROT, STRANS, frame_time=ft)
    np.testing.assert_allclose(sigma2, rep["sigma2"], rtol=1e-6)
    # odd entries: the gap midpoints; even entries: the smoothed frames (1e-8 in the poses: the solution file's matrix round trip)
    assert np.abs(pose[1::2] - pm).max() <= 1e-8 and np.abs(pose[0::2] - z).max() <= 1e-8
    for k in range(F - 1):
        assert np.abs(blk[2 * k + 1] - rep["sigma2"] * cm[k]).max() <= 1e-6 * np.abs(rep["sigma2"] * cm[k]).max(), k
    for f in range(F):
        assert np.abs(blk[2 * f] - rep["sigma2"] * S[f]).max() <= 1e-6 * np.abs(rep["sigma2"] * S[f]).max(), f
    # without -resample no file is written; refused with the usage message: without -smooth, together with -live, n < 2
    os.remove(os.path.join(folder, "final.resampled.yaml"))
    run = subprocess.run(base + ["-smooth", repr(SROT), repr(STRANS)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "resample: " not in run.stdout and not os.path.exists(os.path.join(folder, "final.resampled.yaml"))
    for bad in (base + ["-resample", "2"], base + ["-live", "0", "-resample", "2"], base + ["-smooth", repr(SROT), repr(STRANS), "-resample", "1"]):
        run = subprocess.run(bad, capture_output=True, text=True, timeout=300)
        assert "Usage:" in run.stdout and "-resample" in run.stdout and "resample: " not in run.stdout, run.stdout
        assert not os.path.exists(os.path.join(folder, "final.resampled.yaml"))
