"""The layers above aar_problem_detection_loo that need no device: aar_loo_write_yaml (and its parser, which the GPU tests use), the usage
errors of aar_find_solution -loo / -reject-loo, MultiCamMapper::gate_detections mapping ids before any device is looked for.  CPU only."""
import os
import re
import subprocess

import numpy as np

import aar
from conftest import PKG, ROOT, load_golden


def parse_loo_yaml(path):
    """dict(scalars, cameras {id: (n, max_f, rejected)}, markers, listed [(frame id, cam id, marker id, F, q, leverage, error)])"""
    num = r"([-+.\w]+)"
    out = dict(cameras={}, markers={}, listed=[])
    sect = None
    lines = open(path).read().splitlines()
    assert lines[0] == "%YAML:1.0" and lines[1] == "---"
    val = lambda s: float("nan") if s == ".nan" else (float("inf") if s == ".inf" else float(s))
    for ln in lines[2:]:
        m = re.match(r"^(\w+):\s*(\S*)$", ln)
        if m and m.group(2):
            out[m.group(1)] = val(m.group(2))
            continue
        if m:
            sect = m.group(1)
            continue
        m = re.match(r"^   - \{ (cam_id|marker_id):(-?\d+), detections:(\d+), max_f: %s, rejected:(\d+) \}$" % num, ln)
        if m:
            out["cameras" if m.group(1) == "cam_id" else "markers"][int(m.group(2))] = (int(m.group(3)), val(m.group(4)), int(m.group(5)))
            assert sect == ("cameras" if m.group(1) == "cam_id" else "markers")
            continue
        m = re.match(r"^   - \{ frame_id:(-?\d+), cam_id:(-?\d+), marker_id:(-?\d+), F: %s, q: %s, leverage: %s, error: %s \}$" % (num, num, num, num), ln)
        assert m and sect == "listed_detections", ln
        out["listed"].append(tuple(int(m.group(k)) for k in (1, 2, 3)) + tuple(val(m.group(k)) for k in (4, 5, 6, 7)))
    return out


def build_loo_mapper_tool(tmp_path):
    exe = str(tmp_path / "loo_mapper_main")
    cc = subprocess.run(["g++", "-O0", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "tools", "loo_mapper_main.cpp"), "-o", exe, "-L" + PKG, "-laar",
                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def _fake_loo(ds, f_max):
    N = ds.num_obs
    rng = np.random.default_rng(7)
    F = rng.uniform(0.0, 3.0, N)
    F[5], F[11] = 9.5, np.inf
    st = np.zeros(N, dtype=np.uint8)
    st[2] = aar.PREDICT_UNDETERMINED
    F[2] = np.nan
    keep = np.where((st == 0) & (F > f_max), 0, 1).astype(np.uint8)
    rep = dict(dof=8 * N - 100, undetermined=1, rejected=int((keep == 0).sum()), f_max=f_max, max_f=np.inf, argmax_f=11,
               predict=dict(num_residuals=8 * N, num_vars=100, sum_sq=12.5, sigma2=0.25, num_live_vars=94, leverage_sum=94.0, undefined=0, behind=0,
                            launches=3, seconds=0.001))
    return aar.DetectionLoo(F=F, q=8 * F * 0.25, leverage=rng.uniform(0.1, 4.0, N), status=st, keep=keep, report=rep)


def test_loo_yaml_round_trip(tmp_path):
    ds, _ = load_golden("g2_small")
    loo = _fake_loo(ds, 4.0)
    err = np.linspace(0.1, 2.0, ds.num_obs)
    path = str(tmp_path / "loo.yaml")
    aar.loo_write_yaml(path, ds, loo, err)
    y = parse_loo_yaml(path)
    assert (y["sigma2"], y["dof"], y["num_live_vars"], y["f_max"], y["undetermined"], y["rejected"]) == (0.25, 8 * ds.num_obs - 100, 94, 4.0, 1, loo.report["rejected"])
    assert np.isinf(y["max_f"])
    want = np.nonzero((loo.keep == 0) | (loo.status != 0))[0]
    assert want.tolist() == [2, 5, 11]
    assert len(y["listed"]) == len(want)
    for row, o in zip(y["listed"], want):
        assert row[:3] == (int(ds.frame_ids[ds.obs_frame[o]]), int(ds.cam_ids[ds.obs_cam[o]]), int(ds.marker_ids[ds.obs_marker[o]]))
        np.testing.assert_allclose(row[3:], (loo.F[o], loo.q[o], loo.leverage[o], err[o]), rtol=1e-6)
    for k, c in enumerate(ds.cam_ids):
        sel = np.asarray(ds.obs_cam) == k
        n, mx, rej = y["cameras"][int(c)]
        f = loo.F[sel][~np.isnan(loo.F[sel])]
        assert n == sel.sum() and rej == int((loo.keep[sel] == 0).sum())
        np.testing.assert_allclose(mx, f.max() if len(f) else 0.0, rtol=1e-6)
    assert sum(v[0] for v in y["markers"].values()) == ds.num_obs
    assert aar.lib().aar_loo_write_yaml(path.encode(), None, None, None, None, None, None, None, None) == aar.AAR_ERR_INVALID


def test_find_solution_loo_usage_errors(tmp_path):
    exe = os.path.join(PKG, "aar_find_solution")
    folder = str(tmp_path / "run")
    for bad in (["-loo"], ["-loo", "0"], ["-loo", "-2"], ["-reject-loo"], ["-reject-loo", "nan"], ["-loo", "3", "-with-huber"],
                ["-with-huber", "-reject-loo", "3"]):
        run = subprocess.run([exe, folder, "0.05", "x"] + bad, capture_output=True, text=True)
        assert run.returncode != 0 and "-reject-loo" in run.stdout, bad          # (the usage message, before anything is read)


def test_mapper_gate_maps_ids_and_names_an_unknown_one(tmp_path):
    run = subprocess.run([build_loo_mapper_tool(tmp_path)], capture_output=True, text=True, timeout=120)
    kv = dict(ln.split(" = ", 1) for ln in run.stdout.splitlines() if " = " in ln)
    for what in ("camera", "marker", "frame"):
        assert re.fullmatch(r"MultiCamMapper: no %s with id \d+" % what, kv["unknown_" + what]), kv
    assert "differ in length" in kv["lengths"]
    if aar.device_count() == 0:
        assert run.returncode == 2 and "no CPU path" in kv["device"]
