// The index tables of a problem: see problem_plan.h.  Host arithmetic only.
#include "problem_plan.h"

#include <algorithm>
#include <array>
#include <cstring>
#include <numeric>
#include <utility>

namespace aar {

std::vector<int32_t> plan_held_entities(const PoseLayout &L, const aar_problem_constraints *cons) {
    std::vector<int32_t> held(L.C + L.M, 0);
    if (cons) {
        for (int i = 0; i < cons->n_fixed_cams; i++) { const int c = cons->fixed_cams[i]; if (c != L.rc && L.oc) held[c] = 1; }
        for (int i = 0; i < cons->n_fixed_markers; i++) { const int m = cons->fixed_markers[i]; if (m != L.rm && L.om) held[L.C + m] = 1; }
    }
    return held;
}

// ---- ordering A (reference order) + per-frame slot lists ----
FramePlan plan_frames(const aar_problem_desc &d, const PoseLayout &L, const std::vector<int64_t> &per_frame, int f_begin, int f_end, int64_t ob) {
    FramePlan fp;
    const int C = L.C, M = L.M;
    const int A = fp.A = C + M + (L.oi ? C : 0), F = fp.F = f_end - f_begin;
    int64_t N = 0;
    for (int f = f_begin; f < f_end; f++) N += per_frame[f];
    fp.N = N;
    fp.frame_obs_start.assign(F + 1, 0);
    fp.fslot_start.assign(F + 1, 0);
    fp.a_idx.resize(N);
    fp.a_uv.resize((size_t)8 * N);
    if (N) memcpy(fp.a_uv.data(), d.obs_uv + 8 * ob, sizeof(float) * 8 * N);
    {
        int64_t o = 0;
        std::vector<int32_t> slot_of(A, -1);
        for (int f = 0; f < F; f++) {
            fp.frame_obs_start[f] = (int32_t)o;
            const int64_t cnt = per_frame[f_begin + f];
            std::vector<int32_t> ents;
            for (int64_t k = 0; k < cnt; k++) {
                const int64_t g = ob + o + k;
                ents.push_back(d.obs_cam[g]);
                ents.push_back(C + d.obs_marker[g]);
                if (L.oi) ents.push_back(C + M + d.obs_cam[g]);
            }
            std::sort(ents.begin(), ents.end());
            ents.erase(std::unique(ents.begin(), ents.end()), ents.end());
            if (ents.size() >= (1u << SLOT_C_BITS) && !fp.status) fp.status = set_error(AAR_ERR_UNSUPPORTED, "frame %d touches %zu entities (limit %d)", f, ents.size(), (1 << SLOT_C_BITS) - 1);
            for (size_t s = 0; s < ents.size(); s++) slot_of[ents[s]] = (int32_t)s;
            for (int64_t k = 0; k < cnt; k++) {
                const int64_t g = ob + o + k;
                ObsIdx id;
                id.frame = f; id.cam = d.obs_cam[g]; id.marker = C + d.obs_marker[g];
                id.slots = pack_slots(slot_of[id.cam], slot_of[id.marker], L.oi ? slot_of[C + M + id.cam] : 0);
                fp.a_idx[o + k] = id;
            }
            fp.fslot_start[f] = (int32_t)fp.fslot_ent.size();
            fp.fslot_ent.insert(fp.fslot_ent.end(), ents.begin(), ents.end());
            fp.max_kf = std::max<int>(fp.max_kf, (int)ents.size());
            o += cnt;
        }
        fp.frame_obs_start[F] = (int32_t)o;
        fp.fslot_start[F] = (int32_t)fp.fslot_ent.size();
    }
    fp.total_slots = (int)fp.fslot_ent.size();
    fp.frame_stride.assign(F, 1);   // the observations of a frame are camera-major: a stride of ~ n / 8, coprime with n, puts different cameras into neighbouring lanes
    for (int f = 0; f < F; f++) {
        const int n = fp.frame_obs_start[f + 1] - fp.frame_obs_start[f];
        if (n <= 16) continue;
        int st = n / 8 + 1;
        while (std::gcd(st, n) != 1) st++;
        fp.frame_stride[f] = st;
    }
    return fp;
}

OrderingB plan_ordering_b(const ObsIdx *a_idx, int64_t N) {
    OrderingB B;
    B.perm.resize(N);
    std::iota(B.perm.begin(), B.perm.end(), 0);
    std::stable_sort(B.perm.begin(), B.perm.end(), [&](int32_t x, int32_t y) {
        const ObsIdx &p = a_idx[x], &q = a_idx[y];
        if (p.cam != q.cam) return p.cam < q.cam;
        if (p.marker != q.marker) return p.marker < q.marker;
        return p.frame < q.frame;
    });
    for (int64_t i = 0; i < N;) {
        const ObsIdx &h = a_idx[B.perm[i]];
        int64_t e = i;
        while (e < N && a_idx[B.perm[e]].cam == h.cam && a_idx[B.perm[e]].marker == h.marker) e++;
        B.run_start.push_back((int32_t)i);
        i = e;
    }
    B.run_start.push_back((int32_t)N);
    return B;
}

namespace {

// (entity, frame) incidence, per entity frame-ascending: {frame, W block}; pair_base[a]: entity a's first record in pair_rec
typedef std::vector<std::vector<std::pair<int32_t, int32_t>>> Incidence;

// ---- ordering B: (camera, marker, frame) runs cut into wave-sized chunks ----
void plan_chunks(const FramePlan &fp, const PlanKnobs &knobs, TablePlan &T) {
    const int64_t N = fp.N;
    const OrderingB B = plan_ordering_b(fp.a_idx.data(), N);
    T.b_idx.resize(N);
    T.b_uv.resize((size_t)8 * N);
    for (int64_t i = 0; i < N; i++) {
        T.b_idx[i] = fp.a_idx[B.perm[i]];
        memcpy(&T.b_uv[8 * i], &fp.a_uv[8 * (size_t)B.perm[i]], 8 * sizeof(float));
    }
    // (a wavefront pays a wave sum of 90 values and 90 atomics per chunk whatever its length: config 5's runs of ~390 observations as ONE chunk each, 3 200 wavefronts,
    //  run 11 % faster than cut at 256 -- profiles/r04_attempts.txt section 17; small problems keep 64 and the parallelism)
    int chunk_len = (int)((N / 2048 + 63) / 64 * 64);
    chunk_len = std::min(std::max(chunk_len, 64), 512);
    if (knobs.passb_chunk) chunk_len = std::min(std::max(*knobs.passb_chunk / 64 * 64, 64), PASSB_CHUNK);   // tuning knob (observations of a run per wavefront)
    for (size_t r = 0; r + 1 < B.run_start.size(); r++)
        for (int64_t s = B.run_start[r]; s < B.run_start[r + 1]; s += chunk_len) T.chunk_start.push_back((int32_t)s);
    T.n_chunks = (int)T.chunk_start.size();
    T.chunk_start.push_back((int32_t)N);
}

// ---- which off-diagonal blocks of U exist: entities that share an observation (camera x marker; with intrinsics entities also those of the camera) ----
void plan_neighbours(const PoseLayout &L, int A, const aar_problem_constraints *cons, const std::vector<int32_t> &held, TablePlan &T) {
    const int C = L.C, M = L.M;
    auto pair_end_fixed = [&](int e) { return held[e] || (e < C ? (e == L.rc || !L.oc) : (e - C == L.rm || !L.om)); };   // (e: a camera or marker entity)
    const std::vector<ObsIdx> &b_idx = T.b_idx;
    const std::vector<int32_t> &chunk_start = T.chunk_start;
    std::vector<int32_t> &up_start = T.up_start, &up_ent = T.up_ent;
    up_start.assign(A + 1, 0);
    std::vector<std::vector<int32_t>> nb(A);
    for (int ch = 0; ch < T.n_chunks; ch++) {
        const ObsIdx &h = b_idx[chunk_start[ch]];
        if (ch > 0 && b_idx[chunk_start[ch - 1]].cam == h.cam && b_idx[chunk_start[ch - 1]].marker == h.marker) continue;
        int ents[3] = {h.cam, h.marker, L.oi ? C + M + h.cam : -1};
        for (int x = 0; x < 3; x++)
            for (int y = 0; y < 3; y++)
                if (x != y && ents[x] >= 0 && ents[y] >= 0) nb[ents[x]].push_back(ents[y]);
    }
    // relative pose priors: the camera-camera / marker-marker block of a pair whose two ends are free (a fixed end has no block)
    for (int p = 0; cons && p < cons->n_pair_priors; p++) {
        const aar_pair_prior &q = cons->pair_priors[p];
        const int off = q.kind == AAR_PRIOR_CAMERA ? 0 : C, ea = off + q.index_a, eb = off + q.index_b;
        if (pair_end_fixed(ea) || pair_end_fixed(eb)) continue;
        nb[ea].push_back(eb);
        nb[eb].push_back(ea);
    }
    for (int a = 0; a < A; a++) {
        std::sort(nb[a].begin(), nb[a].end());
        nb[a].erase(std::unique(nb[a].begin(), nb[a].end()), nb[a].end());
        up_start[a] = (int32_t)up_ent.size();
        up_ent.insert(up_ent.end(), nb[a].begin(), nb[a].end());
    }
    up_start[A] = (int32_t)up_ent.size();
    if (up_ent.empty()) up_ent.push_back(0);
}

// ---- (entity, frame) incidence for the Schur complement, and its work list: plain, frame-window or XCD-interleaved ----
void plan_schur_worklist(const FramePlan &fp, const PlanKnobs &knobs, const Incidence &inc, std::vector<int> &pair_base, TablePlan &T) {
    const int A = fp.A, F = fp.F;
    const std::vector<int32_t> &fslot_start = fp.fslot_start;
    std::vector<PairRec> &pair_rec = T.pair_rec;
    std::vector<int32_t> &sw_ent = T.sw_ent, &sw_begin = T.sw_begin, &sw_end = T.sw_end;
    const int64_t total_pairs = fp.total_slots;
    // (entity, frame) pairs per workgroup: measured optimum 16 (config 3) ... 64 (configs 4, 5); every workgroup ends with
    // an atomic flush of its row panel, so fewer, longer items win once the grid is large enough to fill the chip
    int per_item = (int)std::min<int64_t>(64, std::max<int64_t>(16, total_pairs / 1024));
    per_item = (per_item + 3) / 4 * 4;
    if (knobs.schur_item) per_item = std::max(4, *knobs.schur_item);  // tuning knob (pairs per workgroup)
    pair_base.assign(A + 1, 0);
    for (int a = 0; a < A; a++) {
        pair_base[a] = (int)pair_rec.size();
        for (auto &pr : inc[a]) pair_rec.push_back(PairRec{pr.first, pr.second, fslot_start[pr.first], 0});
    }
    pair_base[A] = (int)pair_rec.size();
    // Large problems (the kernel is then bound by re-reading W blocks): items are cut by FRAME WINDOW and ordered window-major,
    // so that the workgroups in flight at any time walk the same frames and find each other's W blocks in L2 / MALL.
    // Small problems: plain runs of per_item pairs, entity-major (fewer, fuller workgroups).
    int window = 0;
    if (total_pairs >= 262144) window = 64;
    if (knobs.schur_window) window = std::max(0, *knobs.schur_window);
    if (window > 0) {
        std::vector<int> cursor(A, 0);
        for (int f0 = 0; f0 < F; f0 += window)
            for (int a = 0; a < A; a++) {
                int c = cursor[a];
                const int cnt = (int)inc[a].size();
                int e = c;
                while (e < cnt && inc[a][e].first < f0 + window) e++;
                if (e > c) {
                    sw_ent.push_back(a);
                    sw_begin.push_back(pair_base[a] + c);
                    sw_end.push_back(pair_base[a] + e);
                }
                cursor[a] = e;
            }
    } else {
        // XCD-aware order (opt-in, AAR_SCHUR_XCD=1).  Workgroups are dealt round-robin over the 8 XCDs, each with its own L2: with entity-major items every
        // XCD ends up walking ALL frames and pulls the whole of W through its L2 (8 x 3.6 MB per launch at config 3 for 0.67 MB of output).  Here the frames
        // are cut into 8 contiguous ranges instead, an item stays inside one range, and the items of range x sit at positions = x (mod 8): an XCD then
        // only ever touches an eighth of W (holes are padded with empty items; the launch's rider shifts every range by the same XCD).  Measured (round 4,
        // profiles/r04_attempts.txt): k_schur 20.9 -> 20.3 us at config 3, 51.7 -> 59.4 us at config 4 (more, shorter items; every one ends with an atomic
        // flush of its row panel): the kernel is not bound by those fetches -- not the default.
        int xcd = 1;
        if (knobs.schur_xcd) xcd = *knobs.schur_xcd != 0 ? 8 : 1;
        std::vector<std::vector<std::array<int32_t, 3>>> lists(xcd);
        for (int a = 0; a < A; a++) {
            const int cnt = (int)inc[a].size();
            int s = 0;
            for (int x = 0; x < xcd; x++) {
                const int f_hi = (int)((int64_t)F * (x + 1) / xcd);
                int e = s;
                while (e < cnt && inc[a][e].first < f_hi) e++;
                for (int c = s; c < e; c += per_item)
                    lists[x].push_back({(int32_t)a, (int32_t)(pair_base[a] + c), (int32_t)(pair_base[a] + std::min(e, c + per_item))});
                s = e;
            }
        }
        size_t longest = 0;
        for (auto &l : lists) longest = std::max(longest, l.size());
        for (size_t k = 0; k < longest; k++)
            for (int x = 0; x < xcd; x++) {
                if (k < lists[x].size()) { sw_ent.push_back(lists[x][k][0]); sw_begin.push_back(lists[x][k][1]); sw_end.push_back(lists[x][k][2]); }
                else if (xcd > 1) { sw_ent.push_back(0); sw_begin.push_back(0); sw_end.push_back(0); }   // a hole: nothing to walk, an empty panel to flush
            }
    }
    T.n_swork = (int)sw_ent.size();
}

// deterministic mode: a record per Schur work item, the items of every entity in ascending frame order; a record per
// pass-B chunk, the chunks of every camera / marker / (camera, marker) pair in ascending order
void plan_deterministic(const PoseLayout &L, int A, TablePlan &T) {
    const int C = L.C;
    const std::vector<ObsIdx> &b_idx = T.b_idx;
    const std::vector<int32_t> &chunk_start = T.chunk_start, &sw_ent = T.sw_ent, &sw_begin = T.sw_begin;
    std::vector<int32_t> &se_start = T.se_start, &se_items = T.se_items, &pbr_start = T.pbr_start, &pbr_chunk = T.pbr_chunk, &pbr_kind = T.pbr_kind, &pbr_a = T.pbr_a, &pbr_b = T.pbr_b;
    T.sp_off.resize(sw_ent.size());
    std::vector<std::vector<int32_t>> items(A);
    for (size_t w = 0; w < sw_ent.size(); w++) {
        T.sp_off[w] = T.sp_total;
        T.sp_total += ((int64_t)(sw_ent[w] + 1) * 36 + 8);
        items[sw_ent[w]].push_back((int32_t)w);
    }
    se_start.assign(A + 1, 0);
    for (int a = 0; a < A; a++) {
        // frame-ascending: an entity's pairs are frame-ascending in pair_rec, so ordering its items by their first pair does it
        std::sort(items[a].begin(), items[a].end(), [&](int32_t x, int32_t y) { return sw_begin[x] < sw_begin[y]; });
        se_start[a] = (int32_t)se_items.size();
        se_items.insert(se_items.end(), items[a].begin(), items[a].end());
    }
    se_start[A] = (int32_t)se_items.size();
    std::vector<std::vector<int32_t>> by_cam(C), by_mk(A);
    pbr_start.push_back(0);
    auto emit = [&](int kind, int ea, int eb, const std::vector<int32_t> &chs) {
        if (chs.empty()) return;
        pbr_chunk.insert(pbr_chunk.end(), chs.begin(), chs.end());
        pbr_start.push_back((int32_t)pbr_chunk.size());
        pbr_kind.push_back(kind); pbr_a.push_back(ea); pbr_b.push_back(eb);
    };
    std::vector<int32_t> run;
    for (int ch = 0; ch < T.n_chunks; ch++) {
        const ObsIdx &h = b_idx[chunk_start[ch]];
        by_cam[h.cam].push_back(ch);
        by_mk[h.marker].push_back(ch);
        run.push_back(ch);
        const bool last = ch + 1 == T.n_chunks || b_idx[chunk_start[ch + 1]].cam != h.cam || b_idx[chunk_start[ch + 1]].marker != h.marker;
        if (last) { emit(2, h.cam, h.marker, run); run.clear(); }
    }
    for (int c = 0; c < C; c++) emit(0, c, 0, by_cam[c]);
    for (int m = 0; m < A; m++) emit(1, m, 0, by_mk[m]);
    T.n_pbr = (int)pbr_kind.size();
    T.pb_stride = L.oi ? 152 : 90;
}

// many shared entities: the MFMA kernel owns 16 x 32-entity blocks of S and streams frame ranges (solve_kernels.hip);
// frame ranges are cut so that the grid is a few workgroups per CU
void plan_mfma(const FramePlan &fp, const PlanKnobs &knobs, const Incidence &inc, TablePlan &T) {
    const int A = fp.A, F = fp.F;
    const std::vector<int32_t> &fslot_start = fp.fslot_start, &fslot_ent = fp.fslot_ent;
    std::vector<int32_t> &sm_ga = T.sm_ga, &sm_gb = T.sm_gb, &sm_fb = T.sm_fb, &sm_fe = T.sm_fe, &slot_frame = T.slot_frame, &slot_dense = T.slot_dense, &dense_ent = T.dense_ent;
    std::vector<int32_t> &sm_frames = T.sm_frames;   // frame lists of the blocks, back to back
    // dense entity 0 = the pseudo entity g_f; then the entities that are seen at all, MOST FREQUENT FIRST (ties: ascending):
    // the often-seen entities form dense groups, the rarely seen ones share groups that whole stretches of frames do not
    // touch at all -- a block of S then only streams the frames in which both of its entity groups are present
    std::vector<int32_t> seen;
    for (int a = 0; a < A; a++)
        if (!inc[a].empty()) seen.push_back(a);
    std::stable_sort(seen.begin(), seen.end(), [&](int32_t x, int32_t y) { return inc[x].size() > inc[y].size(); });
    std::vector<int32_t> dense_of(A, -1);
    dense_ent.push_back(-1);
    for (int32_t a : seen) { dense_of[a] = (int32_t)dense_ent.size(); dense_ent.push_back(a); }
    T.Ad = ((int)dense_ent.size() + 31) / 32 * 32;
    dense_ent.resize(T.Ad, -1);
    const int nga = T.Ad / 16, ngb = T.Ad / 32;
    // frames in which a group of 16 (a side) / 32 (b side) dense entities has anybody present; the pseudo entity is everywhere
    std::vector<std::vector<uint8_t>> pa(nga, std::vector<uint8_t>(F, 0)), pb(ngb, std::vector<uint8_t>(F, 0));
    for (int f = 0; f < F; f++) {
        pa[0][f] = pb[0][f] = 1;
        for (int s = fslot_start[f]; s < fslot_start[f + 1]; s++) {
            const int dd = dense_of[fslot_ent[s]];
            pa[dd / 16][f] = 1;
            pb[dd / 32][f] = 1;
        }
    }
    struct Blk { int ga, gb; std::vector<int32_t> fr; };
    std::vector<Blk> blks;
    int64_t total_steps = 0;
    for (int ga = 0; ga < nga; ga++)
        for (int gb = 0; gb <= (16 * ga + 15) / 32; gb++) {
            Blk bk{ga, gb, {}};
            for (int f = 0; f < F; f++)
                if (pa[ga][f] && pb[gb][f]) bk.fr.push_back(f);
            if (bk.fr.empty()) continue;
            total_steps += ((int64_t)bk.fr.size() + 1) / 2;
            blks.push_back(std::move(bk));
        }
    // cut every block's frame list into pieces of about total / target frames (even lengths: two frames per step), pieces of
    // the same stretch of frames next to each other so that the workgroups in flight share panels in L2
    int target = 12 * (int)blks.size();   // pieces per block: measured optimum at config 5 (8: -1 %, 24: -9 %); AAR_SCHUR_SPLIT overrides
    if (knobs.schur_split) target = std::max(1, *knobs.schur_split) * (int)blks.size();
    const int64_t plen = std::max<int64_t>(16, ((2 * total_steps + target - 1) / target + 3) / 4 * 4);   // whole steps of the kernel's K loop (2 or 4 frames)
    struct Piece { int blk; int64_t b, e; int f0; };
    std::vector<Piece> pieces;
    for (size_t k = 0; k < blks.size(); k++)
        for (int64_t b0 = 0; b0 < (int64_t)blks[k].fr.size(); b0 += plen)
            pieces.push_back({(int)k, b0, std::min<int64_t>(b0 + plen, (int64_t)blks[k].fr.size()), blks[k].fr[b0]});
    std::stable_sort(pieces.begin(), pieces.end(), [](const Piece &x, const Piece &y) { return x.f0 < y.f0; });
    for (const Piece &pc : pieces) {
        sm_ga.push_back(blks[pc.blk].ga); sm_gb.push_back(blks[pc.blk].gb);
        sm_fb.push_back((int32_t)sm_frames.size());
        sm_frames.insert(sm_frames.end(), blks[pc.blk].fr.begin() + pc.b, blks[pc.blk].fr.begin() + pc.e);
        sm_fe.push_back((int32_t)sm_frames.size());
    }
    slot_frame.resize(fp.total_slots);
    slot_dense.resize(fp.total_slots);
    for (int f = 0; f < F; f++)
        for (int s = fslot_start[f]; s < fslot_start[f + 1]; s++) {
            slot_frame[s] = f;
            slot_dense[s] = dense_of[fslot_ent[s]];
        }
    T.n_smwork = (int)sm_ga.size();
}

// solver pcg, balanced work items: at most `chunk` incidences of one entity each, 1 .. 8 items per entity (PCG_MAX_ITEMS)
void plan_pcg_items(const FramePlan &fp, const PlanKnobs &knobs, const std::vector<int> &pair_base, TablePlan &T) {
    const int A = fp.A;
    const int64_t total_pairs = fp.total_slots;
    const int cus = knobs.n_cus;
    int64_t longest = 0;
    for (int a = 0; a < A; a++) longest = std::max<int64_t>(longest, pair_base[a + 1] - pair_base[a]);
    int64_t chunk = std::max<int64_t>(256, (total_pairs + 2LL * cus - 1) / (2LL * cus));
    chunk = std::max<int64_t>(chunk, (longest + 7) / 8);
    if (knobs.pcg_chunk) chunk = std::max<int64_t>((longest + 7) / 8, *knobs.pcg_chunk);
    std::vector<int32_t> &it_ent = T.pcg_it_ent, &it_begin = T.pcg_it_begin, &it_end = T.pcg_it_end, &ent_item_start = T.pcg_ent_item_start;
    ent_item_start.assign(A + 1, 0);
    for (int a = 0; a < A; a++) {
        ent_item_start[a] = (int32_t)it_ent.size();
        const int64_t b0 = pair_base[a], e0 = T.ent_fixed[a] ? pair_base[a] : pair_base[a + 1];
        int64_t b = b0;
        do {
            const int64_t e = std::min<int64_t>(e0, b + chunk);
            it_ent.push_back(a); it_begin.push_back((int32_t)b); it_end.push_back((int32_t)e);
            b = e;
        } while (b < e0);
    }
    ent_item_start[A] = (int32_t)it_ent.size();
    T.pcg_n_items = (int)it_ent.size();
}

// pair priors, per pair: its ends and whether both are free; per free end entity: the (pair, side) items that add to its diagonal block, in ascending pair order
void plan_pair_elements(const PoseLayout &L, const aar_problem_constraints *cons, TablePlan &T) {
    const int C = L.C, M = L.M;
    const int np_ = cons->n_pair_priors;
    std::vector<int32_t> &ends = T.pair_ends, &el_ent = T.pair_el_ent, &el_start = T.pair_el_start, &el_item = T.pair_el_item;
    ends.assign((size_t)np_ * 4, 0);
    std::vector<std::vector<int32_t>> items(C + M);
    for (int p = 0; p < np_; p++) {
        const aar_pair_prior &q = cons->pair_priors[p];
        const int off = q.kind == AAR_PRIOR_CAMERA ? 0 : C, ea = off + q.index_a, eb = off + q.index_b;
        const bool fa = T.ent_fixed[ea] != 0, fb = T.ent_fixed[eb] != 0;
        ends[4 * (size_t)p] = ea; ends[4 * (size_t)p + 1] = eb; ends[4 * (size_t)p + 2] = (!fa && !fb) ? 1 : 0;
        if (!fa) items[ea].push_back(2 * p);
        if (!fb) items[eb].push_back(2 * p + 1);
    }
    for (int e = 0; e < C + M; e++) {
        if (items[e].empty()) continue;
        el_ent.push_back(e);
        el_start.push_back((int32_t)el_item.size());
        el_item.insert(el_item.end(), items[e].begin(), items[e].end());
    }
    el_start.push_back((int32_t)el_item.size());
    T.n_pair_el = (int)el_ent.size();
    T.n_pair_items = (int)el_item.size();
    if (el_ent.empty()) el_ent.push_back(0);
    if (el_item.empty()) el_item.push_back(0);
}

}  // namespace

TablePlan plan_tables(const PoseLayout &L, const FramePlan &fp, const aar_problem_constraints *cons, const PlanKnobs &knobs) {
    TablePlan T;
    const int C = L.C, M = L.M, A = fp.A, F = fp.F;
    const std::vector<int32_t> held = plan_held_entities(L, cons);
    plan_chunks(fp, knobs, T);
    plan_neighbours(L, A, cons, held, T);
    Incidence inc(A);
    for (int f = 0; f < F; f++)
        for (int s = fp.fslot_start[f]; s < fp.fslot_start[f + 1]; s++) inc[fp.fslot_ent[s]].push_back({f, s});
    std::vector<int> pair_base;
    plan_schur_worklist(fp, knobs, inc, pair_base, T);
    if (knobs.deterministic) plan_deterministic(L, A, T);
    if (knobs.schur_mfma && !knobs.use_pcg && F > 0) plan_mfma(fp, knobs, inc, T);   // (problem creation never asks for the MFMA kernel without frames: no block, nothing to cut)
    T.ent_fixed.assign(A, 0);
    for (int c = 0; c < C; c++) T.ent_fixed[c] = (c == L.rc || !L.oc) ? 1 : 0;
    for (int m = 0; m < M; m++) T.ent_fixed[C + m] = (m == L.rm || !L.om) ? 1 : 0;
    for (int e = 0; e < C + M; e++) T.ent_fixed[e] |= held[e];
    // (intrinsics entities are free, root camera included: fill_io_vec_cam_intrinsics covers ALL cameras, libs/multicam_mapper.cpp:488-498;
    //  their two idle parameters have zero rows and columns and get mu on the diagonal, like the reference's five distortion columns)
    if (knobs.use_pcg) plan_pcg_items(fp, knobs, pair_base, T);
    if (cons && cons->n_pair_priors > 0) plan_pair_elements(L, cons, T);
    return T;
}

}  // namespace aar
