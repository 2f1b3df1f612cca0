"""The cases of the problem planner's tables, shared by scripts/record_plan_golden.py (which recorded the tables of the commit before the
planner existed, on the GPU) and tests/test_problem_plan_host.py (which holds host/problem_plan.cpp to them on the CPU).

Every case is aar.synth(3, ...) with small overrides: the smallest shapes at which each branch of the planner is taken.  A case names
  synth        overrides of the generator
  drop_frame   a frame whose observations are removed (a frame with no observation)
  intrinsics / deterministic / solver / fixed_cams / fixed_markers / pair_priors / prior_cams   what the problem is created with
  env          the AAR_* tuning variables of the run
  world, rank  a local group of `world` ranks, the tables of rank `rank`
"""
import numpy as np

GOLDEN_FILE = "plan_parent.npz"
N_CUS = 256   # compute units of the device the golden file was recorded on (only the PCG items' default chunk reads it; the PCG case sets AAR_PCG_CHUNK)

_BASE = dict(synth=dict(num_frames=40), drop_frame=5, intrinsics=False, deterministic=False, solver="direct", env={}, fixed_cams=(), fixed_markers=(),
             pair_priors=(), prior_cams=(), world=1, rank=0)


def _case(**kw):
    c = dict(_BASE)
    c.update(kw)
    return c


CASES = {
    "default": _case(),
    "chunk_cut": _case(synth=dict(num_frames=100, num_cams=2, num_markers=8, min_view_cos=0.01), env={"AAR_PASSB_CHUNK": "64"}),   # (markers seen from nearly any angle: long runs)
    "intrinsics": _case(intrinsics=True),
    "deterministic": _case(deterministic=True),
    "deterministic_intrinsics": _case(deterministic=True, intrinsics=True),
    "window": _case(env={"AAR_SCHUR_WINDOW": "8"}),
    "xcd": _case(env={"AAR_SCHUR_XCD": "1"}),
    "mfma_ad32": _case(synth=dict(num_frames=40, num_cams=4, num_markers=20), env={"AAR_SCHUR_MFMA": "1", "AAR_SCHUR_SPLIT": "4"}),
    "mfma_ad64": _case(env={"AAR_SCHUR_MFMA": "1", "AAR_SCHUR_SPLIT": "4"}),
    "pcg_items": _case(solver="pcg", env={"AAR_PCG_CHUNK": "1"}, fixed_cams=(2,)),
    # ("camera" | "marker", index_a, index_b): both ends free; one end fixed by the caller; one end the root -- and a pose prior on a camera
    "pair_priors": _case(fixed_markers=(3,), pair_priors=(("camera", 1, 2), ("marker", 3, 4), ("camera", 0, 3)), prior_cams=(4,)),
    "sharded": _case(world=2, rank=1),
}

# the variables a case may set, and the planner knob each one feeds (tests/tools/plan_main.cpp reads the knobs by these names)
ENV_KNOBS = {"AAR_PASSB_CHUNK": "passb_chunk", "AAR_SCHUR_ITEM": "schur_item", "AAR_SCHUR_WINDOW": "schur_window", "AAR_SCHUR_XCD": "schur_xcd",
             "AAR_SCHUR_SPLIT": "schur_split", "AAR_PCG_CHUNK": "pcg_chunk"}


def dataset(aar, case):
    """The case's data set (aar: the package)."""
    ds = aar.synth(3, **case["synth"])
    if case["drop_frame"] is not None:
        ds = ds.select_observations(ds.obs_frame != case["drop_frame"])
    return ds


def plan_main_args(case):
    """The case as the key=value arguments of tests/tools/plan_main.cpp."""
    s = case["synth"]
    a = ["frames=%d" % s["num_frames"], "cams=%d" % s.get("num_cams", 0), "markers=%d" % s.get("num_markers", 0),
         "drop_frame=%d" % (-1 if case["drop_frame"] is None else case["drop_frame"]), "intrinsics=%d" % case["intrinsics"],
         "deterministic=%d" % case["deterministic"], "use_pcg=%d" % (case["solver"] == "pcg"),
         "schur_mfma=%d" % (case["env"].get("AAR_SCHUR_MFMA") == "1" or case["solver"] == "pcg"), "n_cus=%d" % N_CUS,
         "world=%d" % case["world"], "rank=%d" % case["rank"]]
    if "min_view_cos" in s:
        a.append("min_view_cos=%r" % s["min_view_cos"])
    for k, v in case["env"].items():
        if k in ENV_KNOBS:
            a.append("%s=%s" % (ENV_KNOBS[k], v))
    a += ["fixed_cam=%d" % c for c in case["fixed_cams"]] + ["fixed_marker=%d" % m for m in case["fixed_markers"]]
    a += ["pair=%s:%d:%d" % (k[0], ia, ib) for k, ia, ib in case["pair_priors"]]
    return a


def read_dump(path):
    """A table dump -> {name: array}.  Records: name [32 bytes, zero padded] | element size int32 | count int64 | the elements.  Elements of
    4 bytes are int32, of 8 int64 (a count of 1: a scalar), of 16 four int32 (ObsIdx, pair_rec)."""
    out = {}
    with open(path, "rb") as f:
        raw = f.read()
    o = 0
    while o < len(raw):
        name = raw[o:o + 32].split(b"\0")[0].decode()
        es = int(np.frombuffer(raw, np.int32, 1, o + 32)[0])
        cnt = int(np.frombuffer(raw, np.int64, 1, o + 36)[0])
        o += 44
        if es == 16:
            v = np.frombuffer(raw, np.int32, 4 * cnt, o).reshape(cnt, 4)
        else:
            v = np.frombuffer(raw, {4: np.int32, 8: np.int64}[es], cnt, o)
        assert name not in out, name
        out[name] = v.copy()
        o += es * cnt
    return out
