// kkt_schedule.cpp -- see kkt_schedule.h.  Host-only: no HIP, no environment.
#include "kkt_schedule.h"

#include <algorithm>
#include <utility>

namespace ipo {

namespace {
int ceil_div(long a, long b) { return static_cast<int>((a + b - 1) / b); }
constexpr int PC = kPanelCols, TR = kTileRows;
// panel workgroups of step t of a tail of nt columns (kkt_dense.hip tail_gp)
int tail_gp(int nt, int t) { return std::max(1, (nt - t * PC + TR - 1) / TR - 1); }
}  // namespace

KktPaths kkt_paths(const KktPlan& P, const KktKnobs& knobs) {
    KktPaths p;
    p.visits = knobs.deep_tree(P.nlevels);
    p.chain_lead = knobs.chain_lead && P.nt > 0 && P.ntb <= kChainMaxBlocks;
    p.tail_blocked = P.nt > 0 && P.ntb > kChainMaxBlocks;
    p.tail_run = knobs.tail_run && P.nt > 0 && P.ntb <= kTailSchedMaxBlocks;
    p.run_winpub = knobs.tail_winpub && p.tail_run;
    p.small_leaves = knobs.small_leaves < 0 ? kSmallLeafMinCount : knobs.small_leaves;
    // Sync-free top levels: from sf_level up every level is at most this many
    // supernodes wide (IPO_HIP_SF_WIDTH): 300 for factors of fewer than 2^25
    // entries, 64 above.  Measured on one box: dfl001 64 / 150 / 300 / 450 /
    // 600 / all -> 290.9 / 292.5 / 292.7 / 292.7 / 292.1 / 224.4 it/s (every
    // level in the launch starves the wide bottom ones), 25fv47 by intpt 932
    // -> 963 at 300; but banded configs[3] 76.9 -> 68.5 and block-angular
    // configs[4] 47.6 -> 39.3 at 300 (their upper levels hold large chunked
    // supernodes, which the per-level launches spread wider).
    p.sf_width = knobs.sf_width > 0 ? knobs.sf_width : P.lx_size < (int64_t(1) << 25) ? 300 : 64;
    return p;
}

// Fused panel units (k_panel_w): per supernode max(1, tiles - 1) workgroups,
// workgroup j holding the diagonal block and 64-row tile j + 1
// (supernodes of at most 16 columns and 64 rows go to the one-wave
// small-panel kernel instead: list small_sups, per level small_ptr)
PanelUnits build_panel_units(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths) {
    PanelUnits r;
    std::vector<int>&fs = r.fu_sup, &fj = r.fu_j, &ss = r.small_sups;
    r.fu_ptr.assign(P.nlevels + 1, 0);
    r.small_ptr.assign(P.nlevels + 1, 0);
    for (int l = 0; l < P.nlevels; l++) {
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; q++) {
            const int sp = P.level_sups[q];
            const int nc = P.col0[sp + 1] - P.col0[sp];
            const int h = nc + P.rowptr[sp + 1] - P.rowptr[sp];
            if (nc <= 16 && h <= kTileRows) { ss.push_back(sp); continue; }
            const int nw = std::max(1, ceil_div(h, kTileRows) - 1);
            for (int j = 0; j < nw; j++) { fs.push_back(sp); fj.push_back(j); }
        }
        r.fu_ptr[l + 1] = static_cast<int>(fs.size());
        r.small_ptr[l + 1] = static_cast<int>(ss.size());
    }
    // Levels whose fused units outnumber their supernodes many times
    // over and fill the device several times (the separator levels of
    // nested dissection: 1,000-3,500 units, 7-14 per supernode) run the
    // per-phase kernels instead: the fused units each refactor their
    // supernode's diagonal block, k_diag factors it once and k_trsm's
    // tiles only read it.  The same operations on every entry in the
    // same order (the IPO_HIP_PANEL=0 path), so bitwise the fused one.
    // IPO_HIP_PANEL_SPLIT: the unit count from which a level splits (0: never)
    const int split_min = knobs.panel_split;
    r.split_level.assign(P.nlevels, 0);
    for (int l = 0; l < P.nlevels && split_min > 0; l++) {
        const int nfu = r.fu_ptr[l + 1] - r.fu_ptr[l];
        int nsup = 0;
        for (int q = r.fu_ptr[l]; q < r.fu_ptr[l + 1]; q++) nsup += fj[q] == 0;
        r.split_level[l] = nfu >= split_min && nfu >= 4 * nsup;
    }
    // single-column small panels of <= 8 rows first in each level's list,
    // eight to a wave (k_panel_s1) on levels of many of them (the leaf
    // sweeps' threshold, IPO_HIP_SMALL_LEAVES)
    r.small1_cnt.assign(P.nlevels, 0);
    const int thr = paths.small_leaves;
    for (int l = 0; l < P.nlevels && thr > 0; l++) {
        const auto b = ss.begin() + r.small_ptr[l], e = ss.begin() + r.small_ptr[l + 1];
        const auto mid = std::stable_partition(b, e, [&](int sp) {
            return P.col0[sp + 1] - P.col0[sp] == 1 && 1 + P.rowptr[sp + 1] - P.rowptr[sp] <= 8;
        });
        if (mid - b >= thr) r.small1_cnt[l] = static_cast<int>(mid - b);
    }
    return r;
}

// Solve chunks: levels holding a panel with more than kChunkRows rows below
// its diagonal block are solved in 64-row chunks (two launches each way)
SolveChunks build_solve_chunks(const KktPlan& P) {
    SolveChunks r;
    std::vector<int>&csup = r.chunk_sup, &cr0 = r.chunk_r0, &chunk0 = r.sup_chunk0;
    chunk0.assign(P.nsup, -1);
    r.chunk_ptr.assign(P.nlevels + 1, 0);
    for (int l = 0; l < P.nlevels; l++) {
        bool big = false;
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; q++) {
            const int sp = P.level_sups[q];
            big |= P.rowptr[sp + 1] - P.rowptr[sp] > kChunkRows;
        }
        if (big)
            for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; q++) {
                const int sp = P.level_sups[q], hb = P.rowptr[sp + 1] - P.rowptr[sp];
                chunk0[sp] = static_cast<int>(csup.size());
                for (int r0 = 0; r0 < hb; r0 += 64) { csup.push_back(sp); cr0.push_back(r0); }
            }
        r.chunk_ptr[l + 1] = static_cast<int>(csup.size());
    }
    r.partial_stride = csup.empty() ? 1 : csup.size() * kPanelCols;
    return r;
}

// Sweep order of each level: on levels without solve chunks the
// single-column supernodes with <= 64 rows below come first (one wave
// each, k_fwd_leaf / k_bwd_leaf), the rest after them.  A blocked tail's
// sweeps take every level by the chunked or the plain kernels: the level order.
SweepOrder build_sweep_order(const KktPlan& P, const KktPaths& paths, const SolveChunks& ch) {
    SweepOrder r;
    std::vector<int>& ss = r.sweep_sups;
    ss = P.level_sups;
    r.leaf_cnt.assign(P.nlevels, 0);
    r.leaf8_cnt.assign(P.nlevels, 0);
    const int min8 = paths.small_leaves;
    for (int l = 0; l < P.nlevels && !paths.tail_blocked; l++) {
        if (ch.chunk_ptr[l + 1] > ch.chunk_ptr[l]) continue;
        const auto b = ss.begin() + P.level_ptr[l], e = ss.begin() + P.level_ptr[l + 1];
        const auto mid = std::stable_partition(b, e, [&](int sp) {
            return P.col0[sp + 1] - P.col0[sp] == 1 && P.rowptr[sp + 1] - P.rowptr[sp] <= 64;
        });
        r.leaf_cnt[l] = static_cast<int>(mid - b);
        if (min8 > 0) {   // the small ones first (k_fwd_leaf8 / k_bwd_leaf8)
            const auto mid8 = std::stable_partition(b, mid, [&](int sp) {
                const int c = P.col0[sp];
                return P.rowptr[sp + 1] - P.rowptr[sp] <= kSmallLeaf &&
                       P.yrow_ptr[c + 1] - P.yrow_ptr[c] <= kSmallLeaf;
            });
            r.leaf8_cnt[l] = static_cast<int>(mid8 - b);
            // a wave of eight leaves touches eight times the cache lines
            // per load: slower on latency-bound levels (dfl001's sweeps
            // 4 ms slower per solve), faster from tens of thousands of
            // leaves on (configs[3]: 10^6)
            if (r.leaf8_cnt[l] < min8) r.leaf8_cnt[l] = 0;
        }
    }
    return r;
}

// Sync-free top levels (k_fwd_sf / k_bwd_sf): from sf_level up every level
// is at most paths.sf_width supernodes wide.  Their forward update values get
// ybuf slices, and their z values zpad slices, of their own 128-B lines;
// work items, per-supernode arrival counts and parents; the forward update
// lists with the moved slices (yrow_idx).
SyncFreePlan build_sync_free_plan(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths,
                                  const SolveChunks& ch) {
    SyncFreePlan r;
    const int kSfWidth = paths.sf_width;
    const int ns = P.nsup, T = P.T;
    int& sf_level = r.sf_level;
    sf_level = P.nlevels;
    while (sf_level > 0 && P.level_ptr[sf_level] - P.level_ptr[sf_level - 1] <= kSfWidth) sf_level--;
    if (P.nlevels - sf_level < 2) sf_level = P.nlevels;
    if (!knobs.sf) sf_level = P.nlevels;
    auto chunked = [&](int sp) { const int l = P.level[sp]; return ch.chunk_ptr[l + 1] > ch.chunk_ptr[l]; };
    auto nchunks = [&](int sp) { return (P.rowptr[sp + 1] - P.rowptr[sp] + 63) / 64; };
    std::vector<int>&ybase = r.ybase, &zbase = r.zbase, &zpi = r.zpi, &need = r.need, &par = r.par;
    ybase.assign(ns + 1, 0);
    zbase.assign(ns, -1);
    zpi.assign(T > 0 ? T : 1, -1);
    need.assign(ns, 0);
    par.assign(ns, -1);
    size_t yend = P.rowptr.empty() ? 0 : P.rowptr.back(), zend = 0;
    for (int sp = 0; sp < ns; sp++) {
        if (P.level[sp] < sf_level) { ybase[sp] = P.rowptr[sp]; continue; }
        yend = (yend + 15) & ~size_t(15);
        ybase[sp] = static_cast<int>(yend);
        yend += P.rowptr[sp + 1] - P.rowptr[sp];
        zend = (zend + 15) & ~size_t(15);
        zbase[sp] = static_cast<int>(zend);
        for (int c = P.col0[sp]; c < P.col0[sp + 1]; c++) zpi[c] = static_cast<int>(zend + c - P.col0[sp]);
        zend += P.col0[sp + 1] - P.col0[sp];
        const int pa = P.parent[sp];
        if (pa >= 0) { par[sp] = pa; need[pa] += chunked(sp) ? nchunks(sp) : 1; }
    }
    ybase[ns] = static_cast<int>(yend);
    std::vector<int>& yidx = r.yrow_idx;
    yidx = P.yrow_idx;
    if (sf_level < P.nlevels) {       // update-value positions of the moved slices
        std::vector<int> pos(yidx.empty() ? 1 : P.rowptr.back());
        for (int sp = 0; sp < ns; sp++)
            for (int i = P.rowptr[sp]; i < P.rowptr[sp + 1]; i++) pos[i] = ybase[sp] + (i - P.rowptr[sp]);
        for (int& e : yidx) e = pos[e];
    }
    // Deep trees: the update values a narrow-range column receives from
    // supernodes below the range (on configs[3] the 10^6 leaves and the wide
    // levels: ~30 scattered values per row, ~5 us of the chain item's loads)
    // are all known once the bottom levels are swept.  They are subtracted
    // from the right-hand side by one pre-pass launch (k_fwd_pre: per column,
    // in list order), and the sync-free items sum only the values of
    // supernodes inside the range (their own lists, ylate_*).
    if (paths.visits && sf_level < P.nlevels) {
        auto src_of = [&](int i) {        // the supernode whose row set holds R entry i
            return static_cast<int>(std::upper_bound(P.rowptr.begin(), P.rowptr.end(), i) - P.rowptr.begin()) - 1;
        };
        r.late_lists = true;
        std::vector<int>&lptr = r.ylate_ptr, &lidx = r.ylate_idx, &ecol = r.pre_col, &eptr = r.pre_ptr,
        &eidx = r.pre_idx;
        lptr.assign(T + 1, 0);
        eptr.assign(1, 0);
        for (int v = 0; v < T; v++) {
            const int sv = v < P.tail_c0 ? P.sup_of[v] : -1;
            const bool in_range = sv >= 0 && P.level[sv] >= sf_level;
            bool any_early = false;
            // (columns outside the range keep empty late lists: only k_fwd_sf reads these)
            for (int e = in_range ? P.yrow_ptr[v] : 0; e < (in_range ? P.yrow_ptr[v + 1] : 0); e++) {
                const bool early = P.level[src_of(P.yrow_idx[e])] < sf_level;
                if (early) {
                    if (!any_early) { ecol.push_back(v); any_early = true; }
                    eidx.push_back(yidx[e]);
                } else {
                    lidx.push_back(yidx[e]);
                }
            }
            if (any_early) eptr.push_back(static_cast<int>(eidx.size()));
            lptr[v + 1] = static_cast<int>(lidx.size());
        }
    }
    r.ybuf_stride = std::max<size_t>(yend, 1);
    std::vector<SchedInt2>&fi = r.items_f, &bi = r.items_b;
    for (int l = sf_level; l < P.nlevels; l++)
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; q++) {
            const int sp = P.level_sups[q];
            if (!chunked(sp)) { fi.push_back({sp, -1}); continue; }
            for (int c = 0; c < nchunks(sp); c++) fi.push_back({sp, ch.sup_chunk0[sp] + c});
        }
    for (int l = P.nlevels - 1; l >= sf_level; l--)
        for (int q = P.level_ptr[l]; q < P.level_ptr[l + 1]; q++) {
            const int sp = P.level_sups[q];
            if (!chunked(sp)) { bi.push_back({sp, -1}); continue; }
            for (int c = 0; c < nchunks(sp); c++) bi.push_back({sp, ch.sup_chunk0[sp] + c});
        }
    r.zpad_stride = std::max<size_t>(zend, 1);
    return r;
}

// Deep elimination trees (at least kVisitLevels levels, e.g. the banded
// BASELINE configs[3]: 2,785 levels, most of them one or two 64-column
// supernodes): a level's gather would wait on every descendant's update,
// although 93 % of its k-slots come from supernodes finished several
// levels earlier.  There each unit's slots are ordered by the level of
// their source (stable), and only the slabs that hold a source of the
// level just below ("late") stay in the unit's own level's gather; the
// earlier slabs become visits of at most kVisitSlots slots, scheduled as
// late as their sources allow into the gather launches of the levels
// below (one visit per unit per launch, each a read-modify-write of the
// unit's tile in slot order).  The level chain then waits per level on
// one small gather and the panel, the visits ride in the same launches
// beside them.  IPO_HIP_VISITS=1/0 forces the schedule on / off
// (KktKnobs::deep_tree); without it the result is empty.
VisitSlots build_visit_slots(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths) {
    VisitSlots v;
    v.vis.resize(P.nlevels + 1);
    if (!paths.visits) return v;
    const int nu = static_cast<int>(P.unit_sup.size());
    const int visit_slabs = knobs.visit_slabs;
    v.kptr.assign(nu + 1, 0);
    v.late_b.assign(nu, 0);
    std::vector<std::pair<int, int>> sl;   // (source level, slot)
    std::vector<int> rl;
    for (int l = 1; l < P.nlevels; l++)
        for (int u = P.unit_level_ptr[l]; u < P.unit_level_ptr[l + 1]; u++) {
            sl.clear();
            for (int i = P.kslot_ptr[u]; i < P.kslot_ptr[u + 1]; i++) {
                const int k = P.kslot[i];
                if (k >= 0) sl.push_back({P.level[P.utasks[k >> 6].src], k});
            }
            std::stable_sort(sl.begin(), sl.end(),
                             [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
            const int kb = static_cast<int>(v.kslot.size());
            rl.clear();
            for (size_t i = 0; i < sl.size(); i++) {
                v.kslot.push_back(sl[i].second);
                if (i % kSlab == 0) rl.push_back(sl[i].first);
                else rl.back() = std::max(rl.back(), sl[i].first);
            }
            while (v.kslot.size() % kSlab) v.kslot.push_back(-1);
            v.kptr[u + 1] = static_cast<int>(v.kslot.size());
            const int nsl = static_cast<int>(rl.size());
            int j = nsl;
            while (j > 0 && rl[j - 1] >= l - 1) j--;
            v.late_b[u] = kb + kSlab * j;
            // early slabs [0, j), backwards, as late as their sources allow
            int t = l - 1, end = j, cur = j;
            while (cur > 0) {
                if (end - cur >= visit_slabs && rl[cur - 1] <= t - 2) {
                    v.vis[t].push_back({u, kb + kSlab * cur, kb + kSlab * end});
                    t--;
                    end = cur;
                }
                cur--;
            }
            if (end > 0) v.vis[t].push_back({u, kb, kb + kSlab * end});
        }
    // groups visit their units in unit order
    for (auto& g : v.vis)
        std::sort(g.begin(), g.end(), [](const SchedInt3& a, const SchedInt3& b) { return a.x < b.x; });
    return v;
}

// Gather chunks (split K): groups = sparse levels (with their visits, vs),
// then the dense tail
GatherChunks build_gather_chunks(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths,
                                 const VisitSlots& vs) {
    GatherChunks r;
    // flat gathers (k_update_flat) for the latency-bound launches of
    // deep trees: IPO_HIP_GATHER_FLAT=0 never, 1 (default) deep trees,
    // 2 every launch of at most kFlatMaxChunks chunks
    const int flat_mode = knobs.gather_flat;
    // quadrant gathers (k_update_quad) on the narrow levels of deep trees
    // (IPO_HIP_GATHER_QUAD=0: off)
    const bool quad_mode = knobs.gather_quad;
    std::vector<int>&cu = r.ck_u, &cb = r.ck_b, &ce = r.ck_e, &cp = r.ck_part, &cq = r.ck_q, &su = r.sp_u,
    &sp0 = r.sp_p0, &sn = r.sp_n;
    r.ck_ptr.assign(P.nlevels + 2, 0);
    r.sp_ptr.assign(P.nlevels + 2, 0);
    size_t max_part = 0;
    const int wg_target = 512;
    const int min_chunk = knobs.min_chunk;
    // units [u0, u1), slots [kbeg(u), kend(u)) each, then the group's visits
    // a sparse unit's 32 x 32 quadrants that hold lower-triangle entries (k_update_quad)
    auto quadrants = [&](int u, int kb, int ke) {
        const int sp = P.unit_sup[u], t = P.unit_tile[u];
        const int nc = P.col0[sp + 1] - P.col0[sp], h = nc + P.rowptr[sp + 1] - P.rowptr[sp];
        const int nrow = std::min(kTileRows, h - t * kTileRows);
        for (int q = 0; q < 4; q++) {
            const int qr = q & 1, qc = q >> 1;
            if (32 * qr >= nrow || 32 * qc >= nc || (t == 0 && qc > qr)) continue;
            cu.push_back(u); cb.push_back(kb); ce.push_back(ke); cp.push_back(-1 - q); cq.push_back(-1);
        }
    };
    auto group = [&](int u0, int u1, auto kbeg, auto kend, const std::vector<SchedInt3>* visits) {
        const long nck0 = static_cast<long>(cu.size());
        long sumk = 0, nun = 0;
        for (int u = u0; u < u1; u++) { sumk += kend(u) - kbeg(u); nun += kend(u) > kbeg(u); }
        // deep trees' narrow levels: quadrant gathers, one chunk per unit
        const bool quad = quad_mode && visits && nun + static_cast<long>(visits->size()) <= kQuadMaxUnits;
        if (quad) {
            for (int u = u0; u < u1; u++)
                if (kend(u) > kbeg(u)) quadrants(u, kbeg(u), kend(u));
            for (const SchedInt3& v : *visits) quadrants(v.x, v.y, v.z);
            r.ck_wide.push_back(false);
            r.ck_kind.push_back(2);
            return;
        }
        // aim at >= wg_target workgroups per launch, chunks of min_chunk..512 slots
        long kmax = (sumk / wg_target + kSlab - 1) / kSlab * kSlab;
        kmax = std::max<long>(min_chunk, std::min<long>(kMaxChunkSlots, kmax));
        int np = 0, mx = 0;
        for (int u = u0; u < u1; u++) {
            const int kb = kbeg(u), ke = kend(u);
            if (ke == kb) continue;
            const int nch = static_cast<int>((ke - kb + kmax - 1) / kmax);
            mx = std::max(mx, nch);
            if (nch > 1) { su.push_back(u); sp0.push_back(np); sn.push_back(nch); }
            for (int j = 0; j < nch; j++) {
                cu.push_back(u);
                cb.push_back(kb + static_cast<int>(j * kmax));
                ce.push_back(std::min<int>(ke, kb + static_cast<int>((j + 1) * kmax)));
                cp.push_back(nch > 1 ? np++ : -1);
                cq.push_back(nch > 1 ? static_cast<int>(su.size()) - 1 : -1);
            }
        }
        if (visits)
            for (const SchedInt3& v : *visits) {
                cu.push_back(v.x); cb.push_back(v.y); ce.push_back(v.z); cp.push_back(-1); cq.push_back(-1);
            }
        max_part = std::max<size_t>(max_part, np);
        // a group of few chunks (about one per CU: occupancy does not
        // matter) whose units are split many ways waits on its partial
        // sums: sum them several at a time
        r.ck_wide.push_back(mx >= 4 && static_cast<long>(cu.size()) - nck0 <= 512);
        r.ck_kind.push_back(quad ? 2 : (flat_mode == 2 || (flat_mode == 1 && paths.visits)) &&
                                               static_cast<long>(cu.size()) - nck0 <= kFlatMaxChunks ? 1 : 0);
    };
    const std::vector<int>& kp = P.kslot_ptr;
    for (int l = 0; l < P.nlevels; l++) {
        if (l == 0) { r.ck_wide.push_back(false); r.ck_kind.push_back(0); }
        else if (paths.visits)
            group(P.unit_level_ptr[l], P.unit_level_ptr[l + 1], [&](int u) { return vs.late_b[u]; },
                  [&](int u) { return vs.kptr[u + 1]; }, &vs.vis[l]);
        else
            group(P.unit_level_ptr[l], P.unit_level_ptr[l + 1], [&](int u) { return kp[u]; },
                  [&](int u) { return kp[u + 1]; }, nullptr);
        r.ck_ptr[l + 1] = static_cast<int>(cu.size());
        r.sp_ptr[l + 1] = static_cast<int>(su.size());
    }
    const std::vector<int>& tp = P.tail_kslot_ptr;
    if (P.nt > 0)
        group(0, P.ntb * (P.ntb + 1) / 2, [&](int u) { return tp[u]; }, [&](int u) { return tp[u + 1]; },
              nullptr);
    else { r.ck_wide.push_back(false); r.ck_kind.push_back(0); }
    r.ck_ptr[P.nlevels + 1] = static_cast<int>(cu.size());
    r.sp_ptr[P.nlevels + 1] = static_cast<int>(su.size());
    r.split_cnt = std::max<size_t>(1, su.size());
    r.partial_tiles = std::max<size_t>(1, max_part);
    return r;
}

int sweep_launches(const std::vector<SweepStep>& steps) {
    int n = 0;
    for (const SweepStep& st : steps) n += st.kind == kSwChunked ? 2 : 1;
    return n;
}

int sweep_split(const std::vector<SweepStep>& fwd) {
    for (size_t i = 0; i + 1 < fwd.size(); i++)
        if (fwd[i].kind == kSwTailGather) return fwd[i + 1].kind == kSwTailLead ? static_cast<int>(i) + 1 : 0;
    return 0;
}

int sweep_lead_end(const std::vector<SweepStep>& fwd) {
    for (size_t i = 0; i < fwd.size(); i++)
        if (fwd[i].kind == kSwTailLead) return static_cast<int>(i) + 1;
    return 0;
}

SweepSteps build_sweep_steps(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths, const SolveChunks& ch,
                             const SweepOrder& order, const SyncFreePlan& sf, bool blocked) {
    SweepSteps r;
    auto level = [&](int l, std::vector<SweepStep>& out) {
        const int q0 = P.level_ptr[l], q1 = P.level_ptr[l + 1];
        const int cb = ch.chunk_ptr[l], ce = ch.chunk_ptr[l + 1];
        if (ce > cb) { out.push_back({kSwChunked, q0, q1 - q0, cb, ce - cb}); return; }
        const int nl = blocked ? 0 : order.leaf_cnt[l], n8 = blocked ? 0 : order.leaf8_cnt[l];
        if (n8 > 0) out.push_back({kSwLeaf8, q0, n8, 0, 0});
        if (nl > n8 && q1 - q0 > nl && knobs.merge_levels) {
            out.push_back({kSwMerged, q0 + n8, nl - n8, q1 - q0 - nl, 0});
        } else {
            if (nl > n8) out.push_back({kSwLeaf, q0 + n8, nl - n8, 0, 0});
            if (q1 - q0 > nl) out.push_back({kSwPlain, q0 + nl, q1 - q0 - nl, 0, 0});
        }
    };
    const bool range = !blocked && sf.range(P);      // the narrow top levels in one launch
    const int top = blocked ? P.nlevels : sf.sf_level;
    const int pre_cols = static_cast<int>(sf.pre_col.size());
    for (int l = 0; l < top; l++) level(l, r.fwd);
    if (range) {
        if (pre_cols > 0) r.fwd.push_back({kSwPre, 0, pre_cols, 0, 0});
        r.fwd.push_back({kSwSyncFree, 0, static_cast<int>(sf.items_f.size()), pre_cols > 0 || sf.late_lists, 0});
    }
    if (P.nt > 0) {
        r.fwd.push_back({kSwTailGather, 0, 0, 0, 0});
        if (blocked) {
            for (int kb = 0; kb < P.ntb; kb++) r.fwd.push_back({kSwTailBlock, 0, 0, kb, 0});
            r.bwd.push_back({kSwTailDscale, 0, 0, 0, 0});
            for (int kb = P.ntb - 1; kb >= 0; kb--) r.bwd.push_back({kSwTailBlock, 0, 0, kb, 0});
        } else {
            r.fwd.push_back({paths.chain_lead ? kSwTailLead : kSwTailChain, 0, 0, 0, 0});
            r.bwd.push_back({knobs.chain_pairs ? kSwTailPair : kSwTailChain, 0, 0, 0, 0});
        }
    }
    if (range) r.bwd.push_back({kSwSyncFree, 0, static_cast<int>(sf.items_b.size()), 0, 0});
    for (int l = top - 1; l >= 0; l--) level(l, r.bwd);
    r.split = sweep_split(r.fwd);
    r.lead_end = sweep_lead_end(r.fwd);
    return r;
}

// Launches per sweep and algorithmic work per phase occurrence
WorkCounts count_work(const KktPlan& P, const KktKnobs& knobs, const SweepSteps& sweep) {
    WorkCounts w;
    w.fwd_launches = sweep_launches(sweep.fwd);
    w.bwd_launches = sweep_launches(sweep.bwd);
    // Bytes: each phase's entries of L read and written once (+ the gather's
    // source reads from the plan)
    double gb = 0;
    auto tasks_bytes = [&](const std::vector<TailTask>& ts) {
        for (const TailTask& t : ts) {
            const double ncd = P.col0[t.src + 1] - P.col0[t.src];
            const double nr = __builtin_popcountll(t.rmask), ncl = __builtin_popcountll(t.cmask);
            gb += 8.0 * ncd * (nr + ncl);
        }
    };
    tasks_bytes(P.utasks);
    tasks_bytes(P.tail_tasks);
    double db = 0, tb = 0, sb = 0;
    for (int sp = 0; sp < P.nsup; sp++) {
        const double nc = P.col0[sp + 1] - P.col0[sp], hb = P.rowptr[sp + 1] - P.rowptr[sp];
        db += 8.0 * 1.5 * nc * nc;
        tb += 16.0 * hb * nc;
        gb += 16.0 * (nc + hb) * nc;      // read-modify-write of every target panel
    }
    const double sdb = db, stb = tb;     // sparse panels alone
    for (int kb = 0; kb < P.ntb; kb++) {
        const double nc = std::min(kPanelCols, P.nt - kb * kPanelCols), below = P.nt - kb * kPanelCols - nc;
        db += 8.0 * 1.5 * nc * nc;
        tb += 16.0 * below * nc;                                // L21 read + write
        const double nb = P.ntb - kb - 1;
        sb += (nb * (nb + 1) / 2) * (16.0 * kTileRows * kTileRows + 16.0 * kTileRows * nc);
    }
    gb += 16.0 * 0.5 * P.nt * P.nt;                                 // tail block read-modify-write
    w.bytes[kPhGather] = gb;
    w.bytes[kPhDiag] = db;
    w.bytes[kPhTrsm] = tb;
    w.bytes[kPhSyrk] = sb;
    // Algorithmic flops per factorisation in SURVEY.md 8(d)'s unit: the
    // reference's narth (ldlt.c:1243-1248), split by the phase doing each
    // column's work (kkt_plan.h: narth_tail / narth_gather / narth_panel,
    // which sum to narth).  What the kernels execute (the plan's flops, the
    // dense tail's explicit zeros) is not the work.
    w.flops[kPhGather] = P.narth_gather;
    if (knobs.panel) {   // k_panel_w does both: the diag phase carries the sparse trsm work;
        // the dense tail is its own phase (k_tail_pr: panels + deferred
        // trailing updates; its repair launches)
        w.flops[kPhDiag] = P.narth_panel; w.bytes[kPhDiag] = sdb + stb;
        w.flops[kPhTrsm] = w.bytes[kPhTrsm] = 0;
        w.flops[kPhSyrk] = w.bytes[kPhSyrk] = 0;
        w.flops[kPhTail] = P.narth_tail;
        w.bytes[kPhTail] = 16.0 * (static_cast<double>(P.lnz_tail) + P.nt);
    } else {            // per-phase path: the tail's work goes with its trailing updates
        w.flops[kPhDiag] = P.narth_panel;
        w.flops[kPhTrsm] = 0;
        w.flops[kPhSyrk] = P.narth_tail;
    }
    // a sweep (s (4 nnz(L) + N) per iteration, a solve
    // being one forward and one backward sweep): 2 nnz(L) + N / 2 flops,
    // every entry of L read once (12 B with its index) and the vector
    // values in and out
    for (int ph : {kPhForward, kPhBackward}) {
        w.flops[ph] = 2.0 * static_cast<double>(P.lnz) + 0.5 * P.T;
        w.bytes[ph] = 12.0 * static_cast<double>(P.lnz) + 16.0 * P.T;
    }
    return w;
}

std::vector<TaskSrc> build_task_src(const KktPlan& P, const std::vector<TailTask>& ts) {
    std::vector<TaskSrc> v(ts.size());
    for (size_t t = 0; t < ts.size(); t++) {
        const int d = ts[t].src, ncd = P.col0[d + 1] - P.col0[d];
        v[t].colbase = P.off[d] + ncd;
        v[t].hd = ncd + (P.rowptr[d + 1] - P.rowptr[d]);
        v[t].cd0 = P.col0[d];
    }
    return v;
}

// per k-slot records of the gather (SlotRec), expanded from the
// slot -> task -> source panel indirection
std::vector<SlotRec> build_slot_records(const KktPlan& P, const std::vector<int>& kslot,
                                        const std::vector<TailTask>& ts) {
    std::vector<SlotRec> v(kslot.size());
    for (size_t i = 0; i < kslot.size(); i++) {
        const int sl = kslot[i];
        SlotRec& r = v[i];
        if (sl < 0) { r.rmask = r.cmask = 0; r.roff = 0; r.cdelta = 0; r.dk = 0; continue; }
        const TailTask& t = ts[sl >> 6];
        const int kl = sl & 63, d = t.src, ncd = P.col0[d + 1] - P.col0[d];
        const int64_t hd = ncd + (P.rowptr[d + 1] - P.rowptr[d]);
        r.rmask = t.rmask;
        r.cmask = t.cmask;
        r.roff = P.off[d] + ncd + kl * hd + t.rbase;
        r.cdelta = t.cbase - t.rbase;
        r.dk = P.col0[d] + kl;
    }
    return v;
}

// ------------------------------------------------ the dense tail's schedules

int tail_visit_tiles(int ntb, int t, int K) {
    int n = 0;
    for (int c = t + 1; c < ntb && visit_hi(t, c, K) > 0; c++) n += ntb - c;
    return t > 0 ? n : 0;
}

// Launch t runs panel t on gp(t) workgroups beside its visits; with one
// workgroup per CU (the kernel's LDS) a launch of more than `cap` workgroups
// takes two rounds of visits: on dfl001 launches 21-37 under visit_hi's
// chunks (up to 286 workgroups, 37-47 us against ~30).  Those launches carry
// the first chunks of later columns' tiles (blocks 0 .. b1 - 1 with b1 <= 6),
// which are ready from launch b1 on: moved, latest-first, into the latest
// earlier launch with room.  Every tile keeps its chunks and their order (its
// first chunk only comes earlier), so the factor is bitwise the same.
std::vector<unsigned> tail_visit_schedule(int ntb, int nt, int K, int cap, bool xcd, std::vector<int>& ptr) {
    struct V { int bi, c, b0, b1; };
    std::vector<std::vector<V>> L(ntb);
    std::vector<int> tot(ntb, 0);
    for (int t = 0; t < ntb; t++) {
        const int h = nt - t * PC;
        tot[t] = std::max(1, (h + TR - 1) / TR - 1);          // launch_tail_step's panel workgroups
        if (t == 0) continue;
        for (int c = t + 1; c < ntb && visit_hi(t, c, K) > 0; c++) {
            const int b1 = visit_hi(t, c, K), b0 = std::max(0, b1 - K);
            for (int bi = c; bi < ntb; bi++) L[t].push_back({bi, c, b0, b1});
        }
        tot[t] += static_cast<int>(L[t].size());
    }
    for (int t = ntb - 1; t > 1; t--) {
        while (tot[t] > cap) {
            // a first chunk of this launch, the one ready earliest (then the
            // farthest column: its tiles have the longest wait before their
            // panel anyway)
            int best = -1;
            for (int q = 0; q < static_cast<int>(L[t].size()); q++) {
                const V& v = L[t][q];
                if (v.b0 != 0) continue;
                if (best < 0 || v.b1 < L[t][best].b1 || (v.b1 == L[t][best].b1 && v.c > L[t][best].c)) best = q;
            }
            if (best < 0) break;
            int dst = -1;
            for (int u = t - 1; u >= std::max(1, L[t][best].b1); u--)
                if (tot[u] < cap) { dst = u; break; }
            if (dst < 0) break;
            L[dst].push_back(L[t][best]);
            tot[dst]++;
            L[t].erase(L[t].begin() + best);
            tot[t]--;
        }
    }
    // XCD grouping (speed only, never correctness): workgroups b and b + 8
    // share an XCD and its L2 (MI355X_MICROARCH.md, round-robin placement),
    // and every visit of column c reads the same blocks L(c, b0 .. b1 - 1)
    // (the B operand, W = L D): the visits of column c go to workgroup ids of
    // one residue mod 8 where possible, so those blocks come from one L2
    // (xcd; KktKnobs::visit_xcd)
    std::vector<unsigned> out;
    ptr.assign(ntb + 1, 0);
    for (int t = 0; t < ntb; t++) {
        ptr[t] = static_cast<int>(out.size());
        std::vector<V> order;
        if (xcd && !L[t].empty()) {
            const int gp = tot[t] - static_cast<int>(L[t].size());
            std::vector<std::vector<V>> q(8);
            for (const V& v : L[t]) q[v.c % 8].push_back(v);
            std::vector<size_t> head(8, 0);
            for (size_t e = 0; e < L[t].size(); e++) {
                int x = (gp + static_cast<int>(e)) % 8;
                if (head[x] == q[x].size()) {           // this residue's columns are used up: the fullest other
                    size_t best = 0;
                    for (int y = 0; y < 8; y++)
                        if (q[y].size() - head[y] > best) { best = q[y].size() - head[y]; x = y; }
                }
                order.push_back(q[x][head[x]++]);
            }
        } else {
            order = L[t];
        }
        for (const V& v : order)
            out.push_back(static_cast<unsigned>(v.bi) | static_cast<unsigned>(v.c) << 8 |
                          static_cast<unsigned>(v.b0) << 16 | static_cast<unsigned>(v.b1) << 24);
    }
    ptr[ntb] = static_cast<int>(out.size());
    return out;
}

// Chunks of column c of the persistent tail, latest first: blocks [0, c - 1)
// (block c - 1 is its panel's pre-update), the latest L blocks one chunk (a
// visit that must finish within one step: it needs block c - 2, final at the
// end of step c - 2, before panel c), then K at a time downwards.
static std::vector<std::pair<int, int>> run_chunks(int c, int K, int L) {
    std::vector<std::pair<int, int>> v;
    int b1 = c - 1;
    for (int k = 0; b1 > 0; k++) {
        const int b0 = std::max(0, b1 - (k == 0 ? L : K));
        v.push_back({b0, b1});
        b1 = b0;
    }
    return v;
}

std::vector<SchedUint2> tail_run_schedule(int ntb, int nt, int K, int L, int cap, std::vector<int>& ptr) {
    // the items hold bi, c, b0, b1, t and the chunk counts in 8 bits each:
    // every caller keeps ntb <= kTailSchedMaxBlocks (the plan constructor,
    // ipo_hip_tail_run_schedule), and a column has at most ntb chunks
    static_assert(kTailSchedMaxBlocks <= 0xff, "tail_run_schedule packs block indices into 8 bits");
    struct V { int bi, c, b0, b1, q; };
    std::vector<std::vector<V>> Ls(ntb);
    std::vector<int> tot(ntb, 0), nch(ntb, 0);
    for (int c = 0; c < ntb; c++) {
        const std::vector<std::pair<int, int>> ch = run_chunks(c, K, L);
        nch[c] = static_cast<int>(ch.size());
        // the k-th chunk from the top in launch c - 1 - k (its blocks < b1 <= c - 1 - k)
        for (int k = 0; k < nch[c]; k++)
            for (int bi = c; bi < ntb; bi++) Ls[c - 1 - k].push_back({bi, c, ch[k].first, ch[k].second, nch[c] - 1 - k});
    }
    for (int t = 0; t < ntb; t++) tot[t] = tail_gp(nt, t) + static_cast<int>(Ls[t].size());
    // launches over `cap` items: first chunks (q = 0) into the latest earlier
    // launch with room where they are ready (launch >= b1), as tail_visit_schedule
    for (int t = ntb - 1; t > 1; t--) {
        while (tot[t] > cap) {
            int best = -1;
            for (int i = 0; i < static_cast<int>(Ls[t].size()); i++) {
                const V& v = Ls[t][i];
                if (v.q != 0) continue;
                if (best < 0 || v.b1 < Ls[t][best].b1 || (v.b1 == Ls[t][best].b1 && v.c > Ls[t][best].c)) best = i;
            }
            if (best < 0) break;
            int dst = -1;
            for (int u = t - 1; u >= std::max(1, Ls[t][best].b1); u--)
                if (tot[u] < cap) { dst = u; break; }
            if (dst < 0) break;
            Ls[dst].push_back(Ls[t][best]);
            tot[dst]++;
            Ls[t].erase(Ls[t].begin() + best);
            tot[t]--;
        }
    }
    std::vector<SchedUint2> out;
    ptr.assign(ntb + 1, 0);
    for (int t = 0; t < ntb; t++) {
        ptr[t] = static_cast<int>(out.size());
        for (int j = 0; j < tail_gp(nt, t); j++)
            out.push_back({static_cast<unsigned>(j), static_cast<unsigned>(t) |
                                                         static_cast<unsigned>(nch[t]) << 8 | 1u << 31});
        // column t + 1's visits first (its panel waits for them), then by column
        std::vector<V>& vv = Ls[t];
        std::stable_sort(vv.begin(), vv.end(), [t](const V& a, const V& b) {
            const bool ua = a.c == t + 1, ub = b.c == t + 1;
            if (ua != ub) return ua;
            return a.c != b.c ? a.c < b.c : a.bi < b.bi;
        });
        for (const V& v : vv)
            out.push_back({static_cast<unsigned>(v.bi) | static_cast<unsigned>(v.c) << 8 |
                               static_cast<unsigned>(v.b0) << 16 | static_cast<unsigned>(v.b1) << 24,
                           static_cast<unsigned>(t) | static_cast<unsigned>(v.q) << 8});
    }
    ptr[ntb] = static_cast<int>(out.size());
    return out;
}

void tail_visit_work(int ntb, int nt, int K, double& flops, double& bytes) {
    flops = bytes = 0.0;
    for (int t = 1; t < ntb; t++)
        for (int c = t + 1; c < ntb && visit_hi(t, c, K) > 0; c++) {
            const int b1 = visit_hi(t, c, K), b0 = std::max(0, b1 - K);
            for (int bi = c; bi < ntb; bi++) {
                const double rows = std::min(TR, nt - bi * TR), cols = std::min(TR, nt - c * TR);
                for (int b = b0; b < b1; b++) {
                    const double k = std::min(PC, nt - b * PC);
                    flops += 2.0 * rows * cols * k;
                    bytes += 8.0 * k * (rows + cols);          // L rows of bi and of c (W = L D formed on load)
                }
                bytes += 16.0 * rows * cols;                   // one read-modify-write of the tile
            }
        }
}

TailSchedule build_tail_schedule(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths, int cus) {
    TailSchedule r;
    if (P.nt <= 0 || P.ntb > kTailSchedMaxBlocks) return r;
    // look-ahead launches of at most one workgroup per CU (tail_visit_schedule)
    if (knobs.visit_sched)
        r.visit_list = tail_visit_schedule(P.ntb, P.nt, knobs.visit_blocks, cus, knobs.visit_xcd, r.visit_ptr);
    // the persistent run (k_tail_run, default; its bails end in the same
    // state as the per-step launches', so the repair and the sharded
    // solve's per-phase redo are unchanged); the latest chunk of each
    // column knobs.visit_latest blocks
    if (paths.tail_run)
        r.run_items = tail_run_schedule(P.ntb, P.nt, knobs.visit_blocks, knobs.visit_latest, cus, r.run_ptr);
    return r;
}

KktSchedule build_kkt_schedule(const KktPlan& P, const KktKnobs& knobs, int cus) {
    KktSchedule s;
    s.paths = kkt_paths(P, knobs);
    s.panels = build_panel_units(P, knobs, s.paths);
    s.chunks = build_solve_chunks(P);
    s.order = build_sweep_order(P, s.paths, s.chunks);
    s.sf = build_sync_free_plan(P, knobs, s.paths, s.chunks);
    s.visits = build_visit_slots(P, knobs, s.paths);
    s.gather = build_gather_chunks(P, knobs, s.paths, s.visits);
    s.sweep = build_sweep_steps(P, knobs, s.paths, s.chunks, s.order, s.sf, s.paths.tail_blocked);
    s.work = count_work(P, knobs, s.sweep);
    s.usrc = build_task_src(P, P.utasks);
    if (P.nt > 0) s.tsrc = build_task_src(P, P.tail_tasks);
    s.slot_rec = build_slot_records(P, s.paths.visits ? s.visits.kslot : P.kslot, P.utasks);
    if (P.nt > 0) s.tail_slot_rec = build_slot_records(P, P.tail_kslot, P.tail_tasks);
    s.tail = build_tail_schedule(P, knobs, s.paths, cus);
    return s;
}

}  // namespace ipo
