"""Every refusal of the smoother's entries, word for word: (entry, model, condition) -> (return code, full text of aar_last_error()) against
tests/golden/smooth_refusals.json, which was recorded once from the library before the driver's two copies of every entry were folded
("The host record").  Code and text are compared exactly.  Needs a real MI355X.

Recording (the library of AAR_LIB, in a process of its own):
    PYTHONPATH=automatic-ar_amd AAR_LIB=.../libaar.so python tests/test_gpu_smooth_refusals.py OUT.json

Not in the table, because no input reaches them through the interface (the fits refuse a problem without detections before their first
E-step, and the elimination's pivot refusal comes before the ones behind it): the M-step variance refusal and the pivot refusals of the two
fits and the fit terms, the pivot refusals of the lag-three blocks, of a query's inverses / eliminations and of the chain's covariance
blocks, and everything a failing HIP call raises.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import aar
import smooth_cases as sc

pytestmark = pytest.mark.gpu

SROT, STRANS = 0.05, 0.02
CV = dict(model="cv", sigma_rot0=0.1, sigma_trans0=0.05)
MODELS = {"rw": dict(), "cv": CV}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smooth_refusals.json")

ENTRIES = ["aar_track_smooth", "aar_track_smooth_system", "aar_track_smooth_system2", "aar_track_smooth_covariance", "aar_track_smooth_covariance2",
           "aar_track_smooth_fit_terms", "aar_track_smooth_fit_terms2", "aar_track_smooth_fit", "aar_track_smooth_fit2", "aar_track_smooth_query",
           "aar_track_smooth_query2", "aar_track_smooth_query2_step", "aar_track_smooth_lag3", "aar_track_smooth_relative"]
RW_ONLY = ["aar_track_smooth_system", "aar_track_smooth_covariance", "aar_track_smooth_fit_terms", "aar_track_smooth_fit", "aar_track_smooth_query"]
CV_ONLY = ["aar_track_smooth_query2_step", "aar_track_smooth_lag3"]
FITS = ["aar_track_smooth_fit_terms", "aar_track_smooth_fit_terms2", "aar_track_smooth_fit", "aar_track_smooth_fit2"]
PIVOTS = ["aar_track_smooth_system", "aar_track_smooth_system2", "aar_track_smooth_covariance", "aar_track_smooth_covariance2",
          "aar_track_smooth_query", "aar_track_smooth_query2", "aar_track_smooth_query2_step", "aar_track_smooth_relative", "aar_track_smooth_lag3"]


def _models(entry):
    return ["rw"] if entry in RW_ONLY else ["cv"] if entry in CV_ONLY else ["rw", "cv"]


def _dataset(F, empty=None):
    """config 2 cut to F frames, as the _shape_dataset helpers of the smoother's tests; empty: the frames without detections"""
    return sc.without_frames(aar.synth(2, num_frames=F), sc.emptied(F) if empty is None else empty)


def _invoke(entry, p, sp, mu=1.0, qt=(0.5,), pairs=((0, 1),), lag2=True, fit=None, null_x=False, null_qt=False, null_fa=False, null_fb=False,
            n=None):
    """one raw call with every output present; sp: aar.SmoothParams or None.  Returns (code, text of aar_last_error())"""
    L, d, ip = aar.lib(), aar._dptr, C.POINTER(C.c_int32)
    F = max(p.ds.num_frames, 1)
    x = np.array(sc.track_start(p.ds), dtype=np.float64)
    xp, s = (None if null_x else d(x)), (None if sp is None else C.byref(sp.c))
    b0, b1, b2, v0, v1, sm = np.zeros((F, 36)), np.zeros((F, 36)), np.zeros((F, 36)), np.zeros(6 * F), np.zeros(6 * F), np.zeros(8)
    q = np.ascontiguousarray(qt, dtype=np.float64)
    fa, fb = aar._pairs(pairs)
    Q = len(fa) if entry.endswith("relative") else len(q)
    o0, o1, o2, seg = np.zeros((max(Q, 1), 36)), np.zeros((max(Q, 1), 36)), np.zeros((max(Q, 1), 36)), np.zeros(max(Q, 1), dtype=np.int32)
    nq = Q if n is None else n
    qp = None if null_qt else d(q)
    path = np.zeros((64, 3))
    args = {
        "aar_track_smooth": (None, s, d(v0), d(v1), None),
        "aar_track_smooth_system": (s, mu, d(b0), d(b1), d(v0), d(v1), d(sm)),
        "aar_track_smooth_system2": (s, mu, d(b0), d(b1), d(b2), d(v0), d(v1), d(sm)),
        "aar_track_smooth_covariance": (s, d(b0), d(b1), None),
        "aar_track_smooth_covariance2": (s, d(b0), d(b1), d(b2) if lag2 else None, None),
        "aar_track_smooth_fit_terms": (s, d(b0), d(sm)),
        "aar_track_smooth_fit_terms2": (s, d(b0), d(sm)),
        "aar_track_smooth_fit": (None, s, None if fit is None else C.byref(fit), d(path), None),
        "aar_track_smooth_fit2": (None, s, None if fit is None else C.byref(fit), d(path), None),
        "aar_track_smooth_query": (s, nq, qp, d(o0), d(o1), seg.ctypes.data_as(ip), None),
        "aar_track_smooth_query2": (s, nq, qp, d(o0), d(o1), seg.ctypes.data_as(ip), None),
        "aar_track_smooth_query2_step": (s, nq, qp, d(o0), d(o1)),
        "aar_track_smooth_lag3": (s, d(b0)),
        "aar_track_smooth_relative": (s, nq, None if null_fa else fa.ctypes.data_as(ip), None if null_fb else fb.ctypes.data_as(ip), d(o0), d(o1), d(o2),
                                      None),
    }[entry]
    code = getattr(L, entry)(p.handle, xp, *args)
    return int(code), L.aar_last_error().decode("utf-8", "replace")


def _params(which, sigma_rot=SROT, **over):
    kw = dict(MODELS[which])
    kw.update(over)
    return aar.SmoothParams(sigma_rot, STRANS, **kw)


def collect():
    """{"entry|model|condition": [code, text]} of every refusal, on the library that aar.lib() has loaded"""
    out = {}
    L = aar.lib()

    def put(entry, model, condition, got):
        out["%s|%s|%s" % (entry, model, condition)] = list(got)

    four = _dataset(4)
    rel4, ft4 = np.full((3, 6), 0.01), np.arange(4.0)
    with aar.Problem(four) as p:
        for e in ENTRIES:
            put(e, "-", "null params", _invoke(e, p, None))
            put(e, "-", "null x_full", _invoke(e, p, _params("rw"), null_x=True))
            put(e, "rw", "struct_size ends before the sigmas", _invoke(e, p, _params("rw", struct_size=aar.CSmoothParams.sigma_trans.offset)))
            put(e, "rw", "sigma_rot = 0", _invoke(e, p, _params("rw", sigma_rot=0.0)))
            put(e, "cv", "rel_motion", _invoke(e, p, _params("cv", rel_motion=rel4)))
        for e in RW_ONLY:
            put(e, "cv", "model", _invoke(e, p, _params("cv")))
        for e in CV_ONLY:
            put(e, "rw", "model", _invoke(e, p, _params("rw", model="rw")))
        put("aar_track_smooth_covariance2", "rw", "lag2_cov", _invoke("aar_track_smooth_covariance2", p, _params("rw")))
        # the parameter checks that every entry shares, through one of them
        e = "aar_track_smooth"
        put(e, "rw", "sigma_trans = -1", _invoke(e, p, aar.SmoothParams(SROT, -1.0)))
        put(e, "rw", "sigma_rot = inf", _invoke(e, p, _params("rw", sigma_rot=np.inf)))
        put(e, "-", "model = 7", _invoke(e, p, _params("rw", model=7)))
        put(e, "cv", "sigma_rot0 = 0", _invoke(e, p, _params("cv", sigma_rot0=0.0)))
        put(e, "cv", "sigma_trans0 = nan", _invoke(e, p, _params("cv", sigma_trans0=np.nan)))
        for model in MODELS:
            put(e, model, "frame_time not finite", _invoke(e, p, _params(model, frame_time=[0.0, 1.0, np.nan, 3.0])))
            put(e, model, "frame_time descends", _invoke(e, p, _params(model, frame_time=[0.0, 2.0, 2.0, 3.0])))
            put(e, model, "frame_time overflows", _invoke(e, p, _params(model, frame_time=[-1.7e308, 1.7e308, 1.75e308, 1.79e308])))
        put(e, "rw", "rel_motion not finite", _invoke(e, p, _params("rw", rel_motion=np.where(np.arange(18) == 8, np.inf, 0.01).reshape(3, 6))))
        for e in ("aar_track_smooth_system", "aar_track_smooth_system2"):
            for model in _models(e):
                put(e, model, "mu = -1", _invoke(e, p, _params(model), mu=-1.0))
                put(e, model, "mu = nan", _invoke(e, p, _params(model), mu=np.nan))
        for e in ("aar_track_smooth_query", "aar_track_smooth_query2", "aar_track_smooth_query2_step"):
            for model in _models(e):
                put(e, model, "query_time not finite", _invoke(e, p, _params(model), qt=[0.5, np.inf]))
                put(e, model, "n_query = -1", _invoke(e, p, _params(model), n=-1))
                put(e, model, "query_time NULL", _invoke(e, p, _params(model), null_qt=True))
                if model == "rw":
                    put(e, model, "rel_motion", _invoke(e, p, _params(model, rel_motion=rel4)))
                    put(e, model, "rel_motion and query_time not finite", _invoke(e, p, _params(model, rel_motion=rel4), qt=[np.nan]))
        e = "aar_track_smooth_relative"
        for model in MODELS:
            put(e, model, "frame_a out of range", _invoke(e, p, _params(model), pairs=[(0, 1), (4, 1)]))
            put(e, model, "frame_b out of range", _invoke(e, p, _params(model), pairs=[(0, -1)]))
            put(e, model, "n_pairs = -1", _invoke(e, p, _params(model), n=-1))
            put(e, model, "frame_a NULL", _invoke(e, p, _params(model), null_fa=True))
            put(e, model, "frame_b NULL", _invoke(e, p, _params(model), null_fb=True))
        for e in ("aar_track_smooth_fit", "aar_track_smooth_fit2"):
            for model in _models(e):
                for name, fp in (("estimate_* all 0", aar.smooth_fit_params(estimate_px=0, estimate_rot=0, estimate_trans=0)),
                                 ("max_iters = 0", aar.smooth_fit_params(max_iters=0)), ("rel_tol = -1", aar.smooth_fit_params(rel_tol=-1.0)),
                                 ("estimate_rot = 2", aar.smooth_fit_params(estimate_rot=2)), ("fit struct_size = 2", aar.smooth_fit_params(struct_size=2))):
                    put(e, model, name, _invoke(e, p, _params(model), fit=fp))
    with aar.Problem(four, with_huber=True) as p:
        for e in FITS:
            for model in _models(e):
                put(e, model, "with_huber", _invoke(e, p, _params(model)))
                put(e, model, "with_huber and estimate_* all 0",
                    _invoke(e, p, _params(model), fit=aar.smooth_fit_params(estimate_px=0, estimate_rot=0, estimate_trans=0)))
    for F in (1, 2):
        with aar.Problem(_dataset(F)) as p:
            for e in FITS:
                for model in _models(e):
                    if F == 1 or model == "cv":
                        put(e, model, "%d frame%s" % (F, "s" * (F > 1)), _invoke(e, p, _params(model)))
    # nothing seen in any frame: the fits refuse the problem, the others their elimination's pivot (a flag the kernels raise, no fault)
    with aar.Problem(_dataset(4, range(4))) as p:
        for e in FITS:
            for model in _models(e):
                put(e, model, "no detections", _invoke(e, p, _params(model)))
        for e in PIVOTS:
            for model in _models(e):
                put(e, model, "pivot", _invoke(e, p, _params(model), mu=0.0, lag2=model == "cv", pairs=[(0, 1), (0, 3)]))
        put("aar_track_smooth_query", "rw", "pivot, frame times", _invoke("aar_track_smooth_query", p, _params("rw", frame_time=ft4), qt=[0.5, 7.0]))
    # behind a communicator, as test_unsupported_behind_a_communicator of the smoother's tests builds it
    group = aar.LocalGroup(1)
    comm = aar.Comm.local(group, 0, 0)
    try:
        with aar.Problem(four, comm=comm) as p:
            for e in ENTRIES:
                for model in MODELS:
                    put(e, model, "communicator", _invoke(e, p, _params(model)))
    finally:
        comm.close()
        group.close()
    # the validators on their own
    sp, qt1, i1 = _params("rw"), np.zeros(1), np.zeros(1, dtype=np.int32)

    def host(name, code):
        put(name, "-", "direct", (int(code), L.aar_last_error().decode("utf-8", "replace")))
    host("aar_smooth_params_validate(NULL)", L.aar_smooth_params_validate(4, None))
    host("aar_smooth_params_validate(num_frames = -1)", L.aar_smooth_params_validate(-1, C.byref(sp.c)))
    host("aar_smooth_query_validate(NULL)", L.aar_smooth_query_validate(4, None, 1, aar._dptr(qt1)))
    host("aar_smooth_query_validate(num_frames = 0)", L.aar_smooth_query_validate(0, C.byref(sp.c), 1, aar._dptr(qt1)))
    host("aar_smooth_relative_validate(NULL)", L.aar_smooth_relative_validate(4, None, 1, i1.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                            i1.ctypes.data_as(C.POINTER(C.c_int32))))
    host("aar_smooth_fit_params_validate(NULL)", L.aar_smooth_fit_params_validate(None))
    return out


@pytest.fixture(scope="module")
def table():
    if aar.device_count() < 1:
        pytest.fail("no HIP device: GPU tests must run on the GPU box (the product has no CPU path)")
    return collect()


def test_every_refusal_is_the_recorded_one(table):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(table) == sorted(want), sorted(set(table) ^ set(want))
    wrong = {k: (table[k], want[k]) for k in want if table[k] != want[k]}
    assert not wrong, wrong


def test_the_table_holds_refusals_only(table):
    # a call that went through would leave the text of the refusal before it: every row is a refusal of its own
    ok = [k for k, (code, text) in table.items() if code == 0 or not text]
    assert not ok, ok
    for k, (code, text) in table.items():
        entry, model, condition = k.split("|")
        if condition == "pivot" or condition.startswith("pivot,"):
            assert code == aar.AAR_ERR_NUMERIC and "non-positive pivot in the block-" in text, (k, code, text)


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(collect(), f, indent=0, sort_keys=True)
        f.write("\n")
