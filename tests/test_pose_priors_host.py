"""Per-entity fixing and pose priors without a GPU: the entry points exist, aar_problem_constraints is size-versioned, every validation
error of aar_problem_constraints_validate names its entry, the compute entry points refuse to run without a device, the CLI parses its new
switches and reads the prior file, and MultiCamMapper maps ids to indices.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aar
from conftest import PKG, ROOT, load_golden

NEW = ("aar_problem_constraints_validate", "aar_problem_create_constrained", "aar_problem_num_priors", "aar_problem_eval_priors")


def test_entry_points_are_exported():
    lib = C.CDLL(aar.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n) and n in aar.SYMBOLS
    assert hasattr(aar.Problem, "eval_priors")
    # include/aar.h layouts: prior = 2 int32 + 42 doubles; constraints = uint32 + int32, ptr, int32 (+pad), ptr, int32 (+pad), ptr
    assert C.sizeof(aar.CPosePrior) == 8 + 42 * 8
    assert C.sizeof(aar.CConstraints) == 48 and aar.CConstraints.priors.offset == 40
    assert aar.NUM_KERNELS == 18 and aar.lib().aar_kernel_name(17).decode() == "k_prior"


def _prior(kind="camera", index=1, info=None, x6=None):
    return (kind, index, np.zeros(6) if x6 is None else x6, np.eye(6) if info is None else info)


def _invalid(ds, match, **kw):
    with pytest.raises(aar.AarError) as e:
        aar.constraints_validate(ds, **kw)
    assert e.value.code == aar.AAR_ERR_INVALID
    assert match in str(e.value), str(e.value)


def test_valid_constraints_pass():
    ds, _ = load_golden("g2_small")
    aar.constraints_validate(ds)
    aar.constraints_validate(ds, fixed_cams=[ds.root_cam], fixed_markers=[ds.root_marker])   # naming a root is allowed
    free_c = [c for c in range(ds.num_cams) if c != ds.root_cam]
    free_m = [m for m in range(ds.num_markers) if m != ds.root_marker]
    aar.constraints_validate(ds, fixed_cams=free_c[:1], priors=[_prior("marker", m) for m in free_m])
    aar.constraints_validate(ds, priors=[_prior("camera", free_c[0], info=np.zeros((6, 6)))])   # L = 0: adds nothing, allowed
    semi = np.diag([1.0, 1.0, 0.0, 4.0, 0.0, 1.0])
    aar.constraints_validate(ds, priors=[_prior("camera", free_c[0], info=semi)])


def test_struct_size_versioning():
    ds, _ = load_golden("g2_small")
    free_c = [c for c in range(ds.num_cams) if c != ds.root_cam]
    bad = [_prior("camera", 99)]
    _invalid(ds, "struct_size", priors=bad, struct_size=0)
    # a caller that knows only the fixed-camera fields: the priors beyond its struct are not read
    aar.constraints_validate(ds, fixed_cams=free_c[:1], priors=bad, struct_size=aar.CConstraints.n_fixed_markers.offset)
    _invalid(ds, "priors[0]", priors=bad, struct_size=C.sizeof(aar.CConstraints))


def test_every_validation_error_names_its_entry():
    ds, _ = load_golden("g2_small")
    C_, M_ = ds.num_cams, ds.num_markers
    c1 = [c for c in range(C_) if c != ds.root_cam][0]
    m1 = [m for m in range(M_) if m != ds.root_marker][0]
    _invalid(ds, "fixed_cams[1] = %d" % C_, fixed_cams=[c1, C_])
    _invalid(ds, "fixed_markers[0] = -1", fixed_markers=[-1])
    _invalid(ds, "priors[0]: camera index %d out of range" % C_, priors=[_prior("camera", C_)])
    _invalid(ds, "priors[1]: marker index -2 out of range", priors=[_prior("camera", c1), _prior("marker", -2)])
    _invalid(ds, "priors[0]: kind 7", priors=[(7, c1, np.zeros(6), np.eye(6))])
    _invalid(ds, "priors[1]: marker index %d already has a prior (priors[0])" % m1, priors=[_prior("marker", m1), _prior("marker", m1)])
    # fixed entities: root, fixed index, non-optimised group
    _invalid(ds, "priors[0]: camera index %d is fixed" % ds.root_cam, priors=[_prior("camera", ds.root_cam)])
    _invalid(ds, "priors[0]: marker index %d is fixed" % ds.root_marker, priors=[_prior("marker", ds.root_marker)])
    _invalid(ds, "priors[0]: camera index %d is fixed" % c1, fixed_cams=[c1], priors=[_prior("camera", c1)])
    _invalid(ds, "priors[0]: marker index %d is fixed" % m1, priors=[_prior("marker", m1)], optimize=(True, False, True))
    # information matrices: indefinite, negative definite, asymmetric, zero pivot over a non-zero column
    _invalid(ds, "priors[0]: the information matrix", priors=[_prior("camera", c1, info=np.diag([1.0, 1, 1, 1, -1, 1]))])
    _invalid(ds, "priors[0]: the information matrix", priors=[_prior("camera", c1, info=-np.eye(6))])
    asym = np.eye(6)
    asym[0, 1] = 0.5
    _invalid(ds, "priors[0]: the information matrix", priors=[_prior("camera", c1, info=asym)])
    zc = np.eye(6)
    zc[2, 2] = 0.0
    zc[2, 4] = zc[4, 2] = 0.5
    _invalid(ds, "priors[0]: the information matrix", priors=[_prior("camera", c1, info=zc)])
    # non-finite values
    x6 = np.zeros(6)
    x6[3] = np.nan
    _invalid(ds, "priors[0]: x6[3] is not finite", priors=[_prior("camera", c1, x6=x6)])
    inf = np.eye(6)
    inf[5, 5] = np.inf
    _invalid(ds, "priors[0]: info[35] is not finite", priors=[_prior("camera", c1, info=inf)])


def test_null_arrays_are_refused():
    ds, _ = load_golden("g2_small")
    cds = ds.as_c()
    d = aar.CProblemDesc()
    aar.lib().aar_problem_desc_from_dataset(C.byref(cds), C.byref(d))
    k = aar.CConstraints()
    k.struct_size = C.sizeof(k)
    k.n_priors = 1
    assert aar.lib().aar_problem_constraints_validate(C.byref(d), C.byref(k)) == aar.AAR_ERR_INVALID
    assert "null array" in aar.lib().aar_last_error().decode()
    assert aar.lib().aar_problem_constraints_validate(C.byref(d), None) == aar.AAR_OK
    assert aar.lib().aar_problem_constraints_validate(None, C.byref(k)) == aar.AAR_ERR_INVALID


@pytest.mark.skipif(aar.device_count() > 0, reason="this check is for machines without a GPU")
def test_compute_entry_points_need_a_device():
    ds, _ = load_golden("g2_small")
    c1 = [c for c in range(ds.num_cams) if c != ds.root_cam][0]
    with pytest.raises(aar.AarError) as e:
        aar.Problem(ds, fixed_cams=[c1], priors=[_prior("marker", [m for m in range(ds.num_markers) if m != ds.root_marker][0])])
    assert e.value.code == aar.AAR_ERR_NO_DEVICE
    # ... but a bad constraint is reported as such before any device is looked for
    with pytest.raises(aar.AarError) as e:
        aar.Problem(ds, priors=[_prior("camera", ds.root_cam)])
    assert e.value.code == aar.AAR_ERR_INVALID
    x = np.zeros(8)
    assert aar.lib().aar_problem_eval_priors(None, x.ctypes.data_as(C.POINTER(C.c_double)), None, None) == aar.AAR_ERR_INVALID
    assert aar.lib().aar_problem_num_priors(None) == 0


def _cli(*args):
    exe = os.path.join(PKG, "aar_find_solution")
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_parses_the_switches_and_reads_the_prior_file(tmp_path):
    folder = str(tmp_path / "s2")
    r = _cli("--synth", 2, folder)
    assert r.returncode == 0, r.stderr
    ds = aar.solution_read(os.path.join(folder, "initial.solution"))
    cid = [int(v) for v in ds.cam_ids]
    mid = [int(v) for v in ds.marker_ids]
    free_c = [cid[c] for c in range(ds.num_cams) if c != ds.root_cam]
    # the fixed cameras take their priors away; the root has none
    r = _cli(folder, 0.05, "x", "-from-initial", "-fix-cams", "%d,%d" % (free_c[0], free_c[1]), "-fix-markers", str(mid[-1]),
             "-prior-solution", os.path.join(folder, "initial.solution"), "-prior-sigma-deg", 0.5, "-prior-sigma-m", 0.002)
    n_pri = (ds.num_cams - 1 - 2) + (ds.num_markers - 1 - (0 if mid[-1] == mid[ds.root_marker] else 1))
    line = "constraints: 2 fixed camera(s), 1 fixed marker(s), %d pose prior(s) from %s (sigma 0.5 deg, 0.002 m)" % (
        n_pri, os.path.join(folder, "initial.solution"))
    assert line in r.stdout, r.stdout + r.stderr
    if aar.device_count() == 0:
        assert r.returncode == 2 and "no CPU path" in r.stderr
    # malformed values: usage
    for bad in (("-fix-cams", "1,x"), ("-fix-markers", ""), ("-prior-sigma-deg", "0"), ("-prior-sigma-m", "-1")):
        r = _cli(folder, 0.05, "x", "-from-initial", *bad)
        assert r.returncode != 0 and "Usage" in r.stdout, bad
    # unknown ids and unreadable prior files end the run before the solve
    r = _cli(folder, 0.05, "x", "-from-initial", "-fix-markers", "99999")
    assert r.returncode == 5 and "no marker with id 99999" in r.stderr
    r = _cli(folder, 0.05, "x", "-from-initial", "-prior-solution", str(tmp_path / "missing.solution"))
    assert r.returncode == 5 and "cannot read the prior solution" in r.stderr


MAPPER_MAIN = r'''
#include <cmath>
#include <cstdio>
#include "multicam_mapper.h"
int main(int argc, char **argv) {
    aar_dataset *d = nullptr;
    if (aar_solution_read(argv[1], &d)) { fprintf(stderr, "%s\n", aar_last_error()); return 1; }
    aar::MultiCamMapper m(d);
    const int C = d->num_cams, M = d->num_markers;
    // ids: the last camera and the last two markers fixed; priors on the first non-root camera and the first non-root marker
    int cfree = d->root_cam == 0 ? 1 : 0, mfree = d->root_marker == 0 ? 1 : 0;
    m.set_fixed_cams({d->cam_ids[C - 1]});
    m.set_fixed_markers({d->marker_ids[M - 1], d->marker_ids[M - 2]});
    std::vector<aar::MultiCamMapper::PosePrior> pr(3);
    pr[0].kind = AAR_PRIOR_CAMERA; pr[0].id = d->cam_ids[cfree];
    pr[1].kind = AAR_PRIOR_MARKER; pr[1].id = d->marker_ids[mfree];
    pr[2].kind = AAR_PRIOR_MARKER; pr[2].id = d->marker_ids[M - 1];   // fixed: left out
    double ang = 0.3;
    for (auto &q : pr) {
        q.T = aar::Mat44{std::cos(ang), -std::sin(ang), 0, 0.1, std::sin(ang), std::cos(ang), 0, -0.2, 0, 0, 1, 0.3, 0, 0, 0, 1};
        for (int i = 0; i < 6; i++) q.info[7 * i] = 2.0;
    }
    m.set_pose_priors(pr);
    aar::MultiCamMapper::ConstraintIndices k = m.constraint_indices();
    printf("fixed_cams");
    for (int c : k.fixed_cams) printf(" %d", c);
    printf("\nfixed_markers");
    for (int v : k.fixed_markers) printf(" %d", v);
    printf("\npriors %zu\n", k.priors.size());
    for (auto &p : k.priors) printf("prior %d %d %.12f %.12f %.12f %.12f %.12f %.12f %.1f\n", p.kind, p.index, p.x6[0], p.x6[1], p.x6[2], p.x6[3], p.x6[4], p.x6[5], p.info[0]);
    m.set_fixed_markers({12345});
    try { m.constraint_indices(); } catch (const std::invalid_argument &e) { printf("error %s\n", e.what()); }
    return 0;
}
'''


def test_mapper_maps_ids_to_indices(tmp_path):
    folder = str(tmp_path / "s2")
    assert _cli("--synth", 2, folder).returncode == 0
    src = tmp_path / "mapper_main.cpp"
    src.write_text(MAPPER_MAIN)
    exe = str(tmp_path / "mapper_main")
    cc = subprocess.run(["g++", "-O0", "-std=c++17", "-I" + os.path.join(PKG, "host"), str(src), "-o", exe, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe, os.path.join(folder, "initial.solution")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    ds = aar.solution_read(os.path.join(folder, "initial.solution"))
    C_, M_ = ds.num_cams, ds.num_markers
    lines = run.stdout.splitlines()
    assert lines[0] == "fixed_cams %d" % (C_ - 1)
    assert lines[1] == "fixed_markers %d %d" % (M_ - 2, M_ - 1)   # (std::set of ids: ascending ids, ascending indices)
    assert lines[2] == "priors 2"
    cfree = 1 if ds.root_cam == 0 else 0
    mfree = 1 if ds.root_marker == 0 else 0
    w = aar.rodrigues_mat2vec(np.array([[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]]))
    for line, kind, idx in zip(lines[3:5], (aar.PRIOR_CAMERA, aar.PRIOR_MARKER), (cfree, mfree)):
        f = line.split()
        assert (int(f[1]), int(f[2])) == (kind, idx)
        np.testing.assert_allclose([float(v) for v in f[3:9]], list(w) + [0.1, -0.2, 0.3], atol=1e-11)
        assert float(f[9]) == 2.0
    assert lines[5] == "error MultiCamMapper: no marker with id 12345"
