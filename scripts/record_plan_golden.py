#!/usr/bin/env python3
"""Writes tests/golden/plan_parent.npz: for every case of tests/plan_cases.py, the integer index tables and counts that problem creation
uploaded, as `<case>/<field>` (a_uv and b_uv are not recorded: the test checks them through the permutation).

It was run ONCE, on the GPU, on the commit before host/problem_plan.cpp existed, when the tables were built inside problem_create of
csrc/ba_capi.hip and could not run without a device.  That commit was patched for the run, and the patched tree thrown away:

    // before `#define UP`
    FILE *plan_dump = getenv("AAR_PLAN_DUMP") ? fopen((std::string(getenv("AAR_PLAN_DUMP")) + (pb->comm ? ".r" + std::to_string(rank) : "")).c_str(), "wb") : nullptr;
    auto dump = [&](const char *name, const auto &vec) {   // (field name, element size, count, bytes); integer tables only
        using T = typename std::decay_t<decltype(vec)>::value_type;
        if (!plan_dump || std::is_floating_point<T>::value) return;
        char nm[32] = {0}; strncpy(nm, name, 31);
        const int32_t es = (int32_t)sizeof(T); const int64_t cnt = (int64_t)vec.size();
        fwrite(nm, 1, 32, plan_dump); fwrite(&es, 4, 1, plan_dump); fwrite(&cnt, 8, 1, plan_dump); if (cnt) fwrite(vec.data(), es, cnt, plan_dump);
    };
    auto dump_count = [&](const char *name, int64_t v) { dump(name, std::vector<int64_t>{v}); };
    #define UP(field, vec) dump(#field, vec); if ((rc = dev_upload(pb, &P.field, vec))) return fail(rc)
    // before the upload of the pair priors' vectors
    dump("pair_ends", ends); dump("pair_el_ent", el_ent); dump("pair_el_start", el_start); dump("pair_el_item", el_item);
    // before `*out = pb`
    dump_count("n_chunks", P.n_chunks); dump_count("n_swork", P.n_swork); dump_count("n_smwork", P.n_smwork); dump_count("Ad", P.Ad); dump_count("max_kf", P.max_kf);
    dump_count("total_slots", P.total_slots); dump_count("n_pbr", P.n_pbr); dump_count("pb_stride", P.pb_stride); dump_count("pcg_n_items", P.pcg_n_items); dump_count("sp_total", sp_total);
    dump_count("n_pair_el", P.n_pair_el); dump_count("n_pair_items", P.n_pair_items);
    if (plan_dump) fclose(plan_dump);

Running it on a later build (which has no such patch) records nothing; patching a later build the same way would only record that build against itself.

    python scripts/record_plan_golden.py [--out FILE]
"""
import argparse
import os
import sys
import tempfile
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "automatic-ar_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import aar  # noqa: E402
import plan_cases as pc  # noqa: E402


def create(case, ds, comm=None):
    eye = np.eye(6)
    kw = dict(solver=case["solver"], deterministic=case["deterministic"], intrinsics=case["intrinsics"], fixed_cams=list(case["fixed_cams"]),
              fixed_markers=list(case["fixed_markers"]), pair_priors=[(k, a, b, np.zeros(6), eye) for k, a, b in case["pair_priors"]],
              priors=[("camera", c, np.zeros(6), eye) for c in case["prior_cams"]], comm=comm)
    aar.Problem(ds, **kw).close()


def record(case, path):
    ds = pc.dataset(aar, case)
    os.environ["AAR_PLAN_DUMP"] = path
    os.environ.update(case["env"])
    try:
        if case["world"] == 1:
            create(case, ds)
            return pc.read_dump(path)
        grp, errs = aar.LocalGroup(case["world"]), []

        def run(rank):
            try:
                comm = aar.Comm.local(grp, rank)
                try:
                    create(case, ds, comm)
                finally:
                    comm.close()
            except Exception as e:      # noqa: BLE001
                errs.append((rank, e))
        th = [threading.Thread(target=run, args=(r,)) for r in range(case["world"])]
        for t in th:
            t.start()
        for t in th:
            t.join()
        grp.close()
        if errs:
            sys.exit("rank %d: %s" % errs[0])
        return pc.read_dump("%s.r%d" % (path, case["rank"]))
    finally:
        for k in list(case["env"]) + ["AAR_PLAN_DUMP"]:
            del os.environ[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", pc.GOLDEN_FILE))
    a = ap.parse_args()
    if aar.device_count() < 1:
        sys.exit("no HIP device")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, case in pc.CASES.items():
            tables = record(case, os.path.join(tmp, name))
            if "n_chunks" not in tables:
                sys.exit("%s: the build wrote no tables (it lacks the recorder's patch)" % name)
            print("%-26s %s" % (name, " ".join("%s=%d" % (k, int(v[0])) for k, v in tables.items() if v.dtype == np.int64 and v.size == 1 and k != "sp_off")), flush=True)
            for k, v in tables.items():
                out["%s/%s" % (name, k)] = v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
