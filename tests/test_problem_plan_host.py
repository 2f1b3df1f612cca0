"""The index tables every kernel walks, built by the host-only planner (host/problem_plan.cpp) on the CPU: tests/tools/plan_main.cpp writes
the tables of every case of tests/plan_cases.py, and this module holds them (1) to the tables the commit before the planner uploaded
(tests/golden/plan_parent.npz, recorded on the GPU by scripts/record_plan_golden.py), entry for entry, and (2) to the invariants the
kernels rely on, restated here in numpy.  CPU only."""
import math
import os
import subprocess

import numpy as np
import pytest

import plan_cases as pc
from conftest import GOLDEN, PKG, ROOT

CASE_NAMES = list(pc.CASES)
SLOT_C_BITS, SLOT_M_BITS, PASSB_CHUNK, PCG_MAX_ITEMS = 10, 11, 1024, 8


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, pc.GOLDEN_FILE))
    out = {name: {} for name in pc.CASES}
    for k in z.files:
        case, field = k.split("/")
        out[case][field] = z[k]
    return out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{case: tables} from ONE build of plan_main and one run per case."""
    tmp = tmp_path_factory.mktemp("plan")
    exe = str(tmp / "plan_main")
    src = [os.path.join(ROOT, "tests", "tools", "plan_main.cpp")] + [os.path.join(PKG, "host", f) for f in ("problem_plan.cpp", "synth.cpp", "dataset.cpp")]
    cc = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + src + ["-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    out = {}
    for name, case in pc.CASES.items():
        path = str(tmp / (name + ".bin"))
        run = subprocess.run([exe, path] + pc.plan_main_args(case), capture_output=True, text=True, timeout=60)
        assert run.returncode == 0, (name, run.stderr[-2000:])
        out[name] = pc.read_dump(path)
    return out


def dims(case):
    """C, M, A of a case"""
    C, M = case["synth"].get("num_cams", 8), case["synth"].get("num_markers", 40)
    return C, M, C + M + (C if case["intrinsics"] else 0)


def scalar(t, k):
    assert t[k].shape == (1,)
    return int(t[k][0])


def runs_of(b_idx):
    """run id of every entry of ordering B, first entry of every (camera, marker) run"""
    if len(b_idx) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    new = np.r_[True, (b_idx[1:, 1] != b_idx[:-1, 1]) | (b_idx[1:, 2] != b_idx[:-1, 2])]
    return np.cumsum(new) - 1, np.flatnonzero(new)


def pair_base(t, A):
    """first record of every entity in pair_rec [A + 1]"""
    ent = t["fslot_ent"][t["pair_rec"][:, 1]]
    return np.searchsorted(ent, np.arange(A + 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal to the parent's tables, entry for entry
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_tables_equal_the_parents(name, plans, golden):
    g, t = golden[name], plans[name]
    assert set(g) == set(t) - {"a_uv_bits", "b_uv_bits"}, sorted(set(g) ^ set(t))
    for k in g:
        assert g[k].dtype == t[k].dtype and g[k].shape == t[k].shape, (k, g[k].dtype, g[k].shape, t[k].dtype, t[k].shape)
        assert np.array_equal(g[k], t[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# the premise of every case, on the golden data itself: a case that stops reaching its branch fails
# ---------------------------------------------------------------------------------------------------------------------------
def test_case_premises_hold_on_the_golden_data(golden):
    g = golden["default"]
    C, M, A = dims(pc.CASES["default"])
    per_frame = np.diff(g["frame_obs_start"])
    assert per_frame.max() > 16 and (g["frame_stride"] != 1).any()            # lane strides other than 1
    assert per_frame[pc.CASES["default"]["drop_frame"]] == 0                  # a frame with no observation
    assert np.setdiff1d(np.arange(C + M), g["fslot_ent"]).size > 0            # an entity no frame sees
    assert g["up_ent"].max() < C + M and np.diff(g["up_start"]).max() >= 2

    g = golden["chunk_cut"]
    rid, first = runs_of(g["b_idx"])
    assert np.bincount(rid).max() > 64 and scalar(g, "n_chunks") > len(first) and np.diff(g["chunk_start"]).max() == 64

    g = golden["intrinsics"]
    C, M, A = dims(pc.CASES["intrinsics"])
    assert (g["a_idx"][:, 3] >> (SLOT_C_BITS + SLOT_M_BITS)).max() > 0 and g["fslot_ent"].max() >= C + M    # the third slot field is used
    assert all(set(g["up_ent"][g["up_start"][c]:g["up_start"][c + 1]]) >= {C + M + c} for c in range(C))     # three-entity neighbour lists

    assert scalar(golden["deterministic"], "pb_stride") == 90 and scalar(golden["deterministic_intrinsics"], "pb_stride") == 152
    for n in ("deterministic", "deterministic_intrinsics"):
        g = golden[n]
        assert scalar(g, "n_pbr") > 0 and scalar(g, "sp_total") > 0 and len(g["se_items"]) == scalar(g, "n_swork") and np.diff(g["se_start"]).max() > 1

    g = golden["window"]
    fr = g["pair_rec"][:, 0]
    assert scalar(g, "n_swork") > scalar(golden["default"], "n_swork")
    assert all(fr[b] // 8 == fr[e - 1] // 8 for b, e in zip(g["sw_begin"], g["sw_end"]))

    g = golden["xcd"]
    assert scalar(g, "n_swork") % 8 == 0 and (g["sw_begin"] == g["sw_end"]).any()          # at least one hole item

    for n, ad in (("mfma_ad32", 32), ("mfma_ad64", 64)):
        g = golden[n]
        assert scalar(g, "Ad") == ad and scalar(g, "n_smwork") > 0
        blocks = set(zip(g["sm_ga"].tolist(), g["sm_gb"].tolist()))
        assert scalar(g, "n_smwork") > len(blocks)                                         # some block has more than one piece

    g = golden["pcg_items"]
    C, M, A = dims(pc.CASES["pcg_items"])
    n_it = np.diff(g["pcg_ent_item_start"])
    assert n_it.max() > 1                                                                  # some entity has more than one item
    fc = pc.CASES["pcg_items"]["fixed_cams"][0]
    i0 = g["pcg_ent_item_start"][fc]
    assert g["ent_fixed"][fc] == 1 and fc in g["fslot_ent"] and n_it[fc] == 1 and g["pcg_it_begin"][i0] == g["pcg_it_end"][i0]   # the empty item of a fixed, seen entity

    g = golden["pair_priors"]
    assert g["pair_ends"].reshape(-1, 4)[:, 2].tolist() == [1, 0, 0] and scalar(g, "n_pair_el") == 4 and scalar(g, "n_pair_items") == 4
    assert 2 in g["up_ent"][g["up_start"][1]:g["up_start"][2]] and 1 in g["up_ent"][g["up_start"][2]:g["up_start"][3]]            # the free pair's block of U

    g, d = golden["sharded"], golden["default"]
    assert 0 < len(g["a_idx"]) < len(d["a_idx"]) and 0 < len(g["fslot_start"]) < len(d["fslot_start"])
    # rank 1's tables are those of the LAST frames: its ordering A is the tail of the whole problem's, frames renumbered from f_begin
    F1, N1 = len(g["fslot_start"]) - 1, len(g["a_idx"])
    f_begin = len(d["fslot_start"]) - 1 - F1
    assert f_begin > 0 and np.array_equal(g["a_idx"][:, 1:3], d["a_idx"][-N1:, 1:3]) and np.array_equal(g["a_idx"][:, 0] + f_begin, d["a_idx"][-N1:, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the invariants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_orderings_chunks_and_slots(name, plans):
    t, case = plans[name], pc.CASES[name]
    C, M, A = dims(case)
    a, b = t["a_idx"], t["b_idx"]
    N, F = len(a), len(t["fslot_start"]) - 1
    # ordering A: frame-major, frame_obs_start its frame boundaries; lane strides coprime with the frame's count
    assert np.all(np.diff(a[:, 0]) >= 0) and np.array_equal(t["frame_obs_start"], np.searchsorted(a[:, 0], np.arange(F + 1)))
    for f, n in enumerate(np.diff(t["frame_obs_start"])):
        st = int(t["frame_stride"][f])
        if n <= 16:
            assert st == 1
        else:
            assert st >= n // 8 + 1 and math.gcd(st, int(n)) == 1 and all(math.gcd(s, int(n)) != 1 for s in range(n // 8 + 1, st))
    # ordering B: a permutation of A, sorted by (camera, marker, frame), stable; the corners follow the same permutation
    perm = np.lexsort((np.arange(N), a[:, 0], a[:, 2], a[:, 1]))
    assert np.array_equal(b, a[perm])
    key = (b[:, 1].astype(np.int64) << 40) + (b[:, 2].astype(np.int64) << 20) + b[:, 0]
    assert np.all(np.diff(key) >= 0)
    assert np.array_equal(t["b_uv_bits"].reshape(N, 8), t["a_uv_bits"].reshape(N, 8)[perm])
    # chunks tile [0, N), never span two runs, never exceed the chunk length (and are cut at multiples of it from the run's start)
    cs = t["chunk_start"]
    chunk_len = min(max((N // 2048 + 63) // 64 * 64, 64), 512)
    if "AAR_PASSB_CHUNK" in case["env"]:
        chunk_len = min(max(int(case["env"]["AAR_PASSB_CHUNK"]) // 64 * 64, 64), PASSB_CHUNK)
    rid, first = runs_of(b)
    assert len(cs) == scalar(t, "n_chunks") + 1 and cs[-1] == N and (N == 0 or cs[0] == 0) and np.all(np.diff(cs) > 0)
    assert np.all(rid[cs[:-1]] == rid[cs[1:] - 1]) and np.diff(cs).max(initial=0) <= chunk_len
    assert np.all((cs[:-1] - first[rid[cs[:-1]]]) % chunk_len == 0) and set(first) <= set(cs[:-1].tolist())
    # slot lists: ascending inside a frame, and the packed slots of every observation index them
    fs, fe = t["fslot_start"], t["fslot_ent"]
    assert fs[0] == 0 and fs[-1] == len(fe) == scalar(t, "total_slots") and np.diff(fs).max() == scalar(t, "max_kf") < (1 << SLOT_C_BITS)
    inside = np.ones(len(fe), bool)
    inside[fs[:-1][np.diff(fs) > 0]] = False
    assert np.all(np.diff(fe)[inside[1:]] > 0) and fe.min() >= 0 and fe.max() < A
    sc, sm, sk = a[:, 3] & ((1 << SLOT_C_BITS) - 1), (a[:, 3] >> SLOT_C_BITS) & ((1 << SLOT_M_BITS) - 1), a[:, 3] >> (SLOT_C_BITS + SLOT_M_BITS)
    base = fs[a[:, 0]]
    assert np.all(base + np.maximum(np.maximum(sc, sm), sk) < fs[a[:, 0] + 1])
    assert np.array_equal(fe[base + sc], a[:, 1]) and np.array_equal(fe[base + sm], a[:, 2]) and a[:, 1].max() < C and a[:, 2].min() >= C
    assert np.array_equal(fe[base + sk], C + M + a[:, 1]) if case["intrinsics"] else np.all(sk == 0)
    # every slot is there because an observation uses it
    used = np.zeros(len(fe), bool)
    used[base + sc] = used[base + sm] = True
    if case["intrinsics"]:
        used[base + sk] = True
    assert used.all()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_incidence_and_schur_work_lists(name, plans):
    t, case = plans[name], pc.CASES[name]
    C, M, A = dims(case)
    fs, fe, pr = t["fslot_start"], t["fslot_ent"], t["pair_rec"]
    F, S = len(fs) - 1, len(fe)
    # pair_rec: every (entity, frame) incidence once, grouped by entity, frame-ascending per entity
    assert np.array_equal(np.sort(pr[:, 1]), np.arange(S)) and np.all(pr[:, 3] == 0)
    assert np.array_equal(pr[:, 2], fs[pr[:, 0]]) and np.all(pr[:, 1] >= fs[pr[:, 0]]) and np.all(pr[:, 1] < fs[pr[:, 0] + 1])
    ent = fe[pr[:, 1]]
    assert np.all(np.diff(ent.astype(np.int64) * (F + 1) + pr[:, 0]) > 0)
    base = pair_base(t, A)
    # the work list: the non-hole items tile every entity's range of pair_rec exactly once
    we, wb, wn = t["sw_ent"], t["sw_begin"], t["sw_end"]
    assert len(we) == len(wb) == len(wn) == scalar(t, "n_swork")
    hole = wb == wn
    assert np.all(we[hole] == 0) and np.all(wb[hole] == 0) and (case["env"].get("AAR_SCHUR_XCD") == "1" or not hole.any())
    o = np.argsort(wb[~hole], kind="stable")
    b_, e_, a_ = wb[~hole][o], wn[~hole][o], we[~hole][o]
    assert b_[0] == 0 and e_[-1] == S and np.array_equal(e_[:-1], b_[1:]) and np.all(e_ > b_)
    assert np.all(base[a_] <= b_) and np.all(e_ <= base[a_ + 1])
    # ... in the shape of the case
    per_item = (min(64, max(16, S // 1024)) + 3) // 4 * 4
    fr = pr[:, 0]
    if "AAR_SCHUR_WINDOW" in case["env"]:
        w = int(case["env"]["AAR_SCHUR_WINDOW"])
        win = fr[wb] // w
        assert np.array_equal(win, fr[wn - 1] // w) and np.all(np.diff(win.astype(np.int64) * A + we) > 0)      # window-major, then entity: one item each
    elif case["env"].get("AAR_SCHUR_XCD") == "1":
        x = np.arange(len(we)) % 8
        lo, hi = F * x // 8, F * (x + 1) // 8
        assert len(we) % 8 == 0 and np.all((wn - wb) <= per_item)
        assert np.all(hole | ((fr[wb] >= lo) & (fr[np.maximum(wn, 1) - 1] < hi)))                                # an item stays inside its XCD's frame range
    else:
        assert np.all(np.diff(wb) > 0) and np.all((wn - wb) <= per_item)                                          # entity-major
        assert np.all(((wn - wb) == per_item) | (wn == base[we + 1]))                                             # only an entity's last item is short
    if case["deterministic"]:
        n_sw = len(we)
        # se_items: a permutation of the items, by entity, frame-ascending per entity; sp_off: the running sum of the items' records
        assert np.array_equal(np.sort(t["se_items"]), np.arange(n_sw)) and t["se_start"][0] == 0 and t["se_start"][-1] == n_sw and len(t["se_start"]) == A + 1
        for a in range(A):
            it = t["se_items"][t["se_start"][a]:t["se_start"][a + 1]]
            assert np.all(we[it] == a) and np.all(np.diff(wb[it]) > 0)
        size = (we.astype(np.int64) + 1) * 36 + 8
        assert t["sp_off"].dtype == np.int64 and np.array_equal(t["sp_off"], np.cumsum(size) - size) and scalar(t, "sp_total") == size.sum()
        # pbr_*: every chunk once per kind, ascending: kind 2 = the (camera, marker) runs in their order, then kind 0 = cameras, kind 1 = marker entities
        b, cs = t["b_idx"], t["chunk_start"][:-1]
        ccam, cmk = b[cs, 1], b[cs, 2]
        rid, _ = runs_of(b)
        expect = [(2, int(ccam[ch[0]]), int(cmk[ch[0]]), ch) for ch in (np.flatnonzero(rid[cs] == r) for r in range(rid[-1] + 1))]
        expect += [(0, c, 0, np.flatnonzero(ccam == c)) for c in range(C) if (ccam == c).any()]
        expect += [(1, m, 0, np.flatnonzero(cmk == m)) for m in range(A) if (cmk == m).any()]
        assert scalar(t, "n_pbr") == len(expect) == len(t["pbr_kind"]) and len(t["pbr_start"]) == len(expect) + 1 and t["pbr_start"][0] == 0
        for i, (kind, ea, eb, ch) in enumerate(expect):
            assert (t["pbr_kind"][i], t["pbr_a"][i], t["pbr_b"][i]) == (kind, ea, eb)
            assert np.array_equal(t["pbr_chunk"][t["pbr_start"][i]:t["pbr_start"][i + 1]], ch)
        for kind in (0, 1, 2):
            got = np.concatenate([t["pbr_chunk"][t["pbr_start"][i]:t["pbr_start"][i + 1]] for i in np.flatnonzero(t["pbr_kind"] == kind)])
            assert np.array_equal(np.sort(got), np.arange(len(cs)))
        assert scalar(t, "pb_stride") == (152 if case["intrinsics"] else 90)
    else:
        assert scalar(t, "n_pbr") == 0 and scalar(t, "sp_total") == 0 and "se_items" not in t


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if n.startswith("mfma")])
def test_mfma_numbering_blocks_and_pieces(name, plans):
    t, case = plans[name], pc.CASES[name]
    C, M, A = dims(case)
    fs, fe = t["fslot_start"], t["fslot_ent"]
    F, Ad = len(fs) - 1, scalar(t, "Ad")
    # dense_ent: the pseudo entity, then the seen entities by frequency (descending), then by index; padded with -1 to a multiple of 32
    cnt = np.bincount(fe, minlength=A)
    seen = [a for a in np.lexsort((np.arange(A), -cnt)) if cnt[a] > 0]
    assert Ad == (len(seen) + 1 + 31) // 32 * 32 and t["dense_ent"].tolist() == [-1] + seen + [-1] * (Ad - 1 - len(seen))
    dense_of = np.full(A, -1)
    dense_of[seen] = 1 + np.arange(len(seen))
    slot_frame = np.repeat(np.arange(F), np.diff(fs))
    assert np.array_equal(t["slot_frame"], slot_frame) and np.array_equal(t["slot_dense"], dense_of[fe])
    # presence of the groups of 16 (a side) and 32 (b side) dense entities per frame; the pseudo entity is in every frame
    pa, pb = np.zeros((Ad // 16, F), bool), np.zeros((Ad // 32, F), bool)
    pa[0], pb[0] = True, True
    pa[t["slot_dense"] // 16, slot_frame] = True
    pb[t["slot_dense"] // 32, slot_frame] = True
    ga, gb, fb, fe_ = t["sm_ga"], t["sm_gb"], t["sm_fb"], t["sm_fe"]
    # the pieces tile sm_frames, ordered by their first frame
    assert fb[0] == 0 and fe_[-1] == len(t["sm_frames"]) and np.array_equal(fe_[:-1], fb[1:]) and np.all(fe_ > fb) and np.all(np.diff(t["sm_frames"][fb]) >= 0)
    blocks = {}
    for w in range(scalar(t, "n_smwork")):
        blocks.setdefault((int(ga[w]), int(gb[w])), []).append(t["sm_frames"][fb[w]:fe_[w]])
    want = {(a, b): np.flatnonzero(pa[a] & pb[b]) for a in range(Ad // 16) for b in range((16 * a + 15) // 32 + 1)}
    want = {k: v for k, v in want.items() if len(v)}
    assert set(blocks) == set(want)
    total_steps = sum((len(v) + 1) // 2 for v in want.values())
    target = max(1, int(case["env"]["AAR_SCHUR_SPLIT"])) * len(want)
    plen = max(16, ((2 * total_steps + target - 1) // target + 3) // 4 * 4)
    for k, pieces in blocks.items():
        assert np.array_equal(np.concatenate(pieces), want[k])                     # exactly the frames where both groups are present, once, ascending
        assert all(len(p) == plen for p in pieces[:-1]) and 0 < len(pieces[-1]) <= plen


@pytest.mark.parametrize("name", CASE_NAMES)
def test_neighbour_lists_fixed_flags_and_pair_elements(name, plans):
    t, case = plans[name], pc.CASES[name]
    C, M, A = dims(case)
    fixed = np.zeros(A, np.int32)
    fixed[0], fixed[C] = 1, 1                      # the roots (camera 0, marker 0 in the generator's data sets)
    fixed[list(case["fixed_cams"])] = 1
    fixed[[C + m for m in case["fixed_markers"]]] = 1
    assert np.array_equal(t["ent_fixed"], fixed)
    us, ue = t["up_start"], t["up_ent"]
    b = t["b_idx"]
    nb = [set() for _ in range(A)]
    for c, m in set(zip(b[:, 1].tolist(), b[:, 2].tolist())):
        group = [c, m] + ([C + M + c] if case["intrinsics"] else [])
        for x in group:
            nb[x] |= set(group) - {x}
    for kind, ia, ib in case["pair_priors"]:
        ea, eb = (ia, ib) if kind == "camera" else (C + ia, C + ib)
        if not fixed[ea] and not fixed[eb]:
            nb[ea].add(eb)
            nb[eb].add(ea)
    assert len(us) == A + 1 and us[0] == 0
    for a in range(A):
        assert ue[us[a]:us[a + 1]].tolist() == sorted(nb[a])                     # sorted, no duplicates, symmetric (nb is)
    assert len(ue) == max(us[-1], 1) and (us[-1] > 0 or ue[0] == 0)
    if case["pair_priors"]:
        ends = t["pair_ends"].reshape(-1, 4)
        items = {}
        for p, (kind, ia, ib) in enumerate(case["pair_priors"]):
            ea, eb = (ia, ib) if kind == "camera" else (C + ia, C + ib)
            assert ends[p].tolist() == [ea, eb, int(not fixed[ea] and not fixed[eb]), 0]
            for side, e in enumerate((ea, eb)):
                if not fixed[e]:
                    items.setdefault(e, []).append(2 * p + side)
        el = sorted(items)
        assert t["pair_el_ent"].tolist() == el and scalar(t, "n_pair_el") == len(el)
        assert t["pair_el_item"].tolist() == [i for e in el for i in items[e]] and scalar(t, "n_pair_items") == len(t["pair_el_item"])
        assert t["pair_el_start"].tolist() == np.r_[0, np.cumsum([len(items[e]) for e in el])].tolist()
    else:
        assert "pair_ends" not in t and scalar(t, "n_pair_el") == 0


def test_pcg_items_tile_the_free_entities(plans):
    t, case = plans["pcg_items"], pc.CASES["pcg_items"]
    C, M, A = dims(case)
    base = pair_base(t, A)
    st, ie, ib, iend = t["pcg_ent_item_start"], t["pcg_it_ent"], t["pcg_it_begin"], t["pcg_it_end"]
    assert len(st) == A + 1 and st[0] == 0 and st[-1] == len(ie) == scalar(t, "pcg_n_items")
    longest = int(np.diff(base).max())
    chunk = max((longest + 7) // 8, int(case["env"]["AAR_PCG_CHUNK"]))
    for a in range(A):
        s, e = st[a], st[a + 1]
        assert 1 <= e - s <= PCG_MAX_ITEMS and np.all(ie[s:e] == a) and ib[s] == base[a]
        if t["ent_fixed"][a] or base[a] == base[a + 1]:
            assert e - s == 1 and iend[s] == ib[s]                                 # a fixed or unseen entity: one empty item
        else:
            assert iend[e - 1] == base[a + 1] and np.array_equal(iend[s:e - 1], ib[s + 1:e]) and np.all(iend[s:e] > ib[s:e]) and np.all(iend[s:e] - ib[s:e] <= chunk)
    for name in CASE_NAMES:
        if name != "pcg_items":
            assert scalar(plans[name], "pcg_n_items") == 0 and "pcg_it_ent" not in plans[name]
