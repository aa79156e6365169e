// kkt_schedule.h -- the launch schedule of a KktDevice as host-only code:
// what the constructor derives from the symbolic plan, the runtime knobs and
// the device's CU count before it uploads anything.  Pure functions, one per
// constructor step, each returning the arrays that step uploads and the few
// counts and flags the launch code reads on the host (KktLaunch).  No HIP, no
// environment: the unit builds with a plain C++17 compiler, so the ordering
// properties the persistent kernels rely on (an item waits only on items
// earlier in its list) are tested on the CPU (tests/test_kkt_schedule.py,
// tests/test_tail_schedule.py).  The dense tail's host schedules live here
// too, and so does the launch list of a substitution sweep (SweepStep,
// build_sweep_steps): which kernels a sweep launches, over which ranges and
// in what order is decided here once, KktDevice::run_sweep_steps
// (kkt_sweep.hip) walks the list, and the launch counts of the timing mode are
// the list's totals.  build_kkt_schedule runs every part in the constructor's
// order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kkt_knobs.h"
#include "kkt_plan.h"

namespace ipo {

constexpr int kSmallLeaf = 8;                  // rows and update values of a small leaf (k_fwd_leaf8 / k_bwd_leaf8)
constexpr int kSmallLeafMinCount = 32768;      // per level, else one wave per leaf
constexpr int kChunkRows = 128;                // a level with a panel of more rows below is solved in 64-row chunks
// the dense-tail sweep chains keep one workgroup per block resident
constexpr int kChainMaxBlocks = 200;
// most block columns of a scheduled tail: the schedules pack block indices
// and chunk counts into 8 bits each (tail_visit_schedule, tail_run_schedule);
// a larger tail takes the per-step launches with the visit_hi formula
constexpr int kTailSchedMaxBlocks = 255;

// Device-time phases of the KKT core (timing mode), with the algorithmic
// work of one occurrence (one factorisation / one substitution sweep).
// kPhTail: the look-ahead dense-tail factor (k_tail_pr and its repair launches).
enum KktPhase { kPhGather = 0, kPhDiag, kPhTrsm, kPhSyrk, kPhForward, kPhBackward, kPhTail, kNumPhases };

// Item pairs and triples, laid out as HIP's int2 / int3 / uint2 (asserted
// where they are uploaded as such)
struct SchedInt2 { int x, y; };
struct SchedInt3 { int x, y, z; };
struct SchedUint2 { unsigned x, y; };

// The paths that the knobs and the plan select together
struct KktPaths {
    bool visits = false;       // the deep-tree gather schedule and the sweeps' pre-pass
    bool chain_lead = false;   // forward dense-tail sweep by one lead workgroup + helpers (k_tail_fwd_lead)
    bool tail_blocked = false; // a tail of more than kChainMaxBlocks block columns: per-block sweep launches
    bool tail_run = false;     // the dense tail as one persistent launch (k_tail_run)
    bool run_winpub = false;   // the run's window hand-off (TailRun::pub)
    int small_leaves = 0;      // knobs.small_leaves, unset: kSmallLeafMinCount
    int sf_width = 0;          // widest level of the sync-free range (build_sync_free_plan)
};
KktPaths kkt_paths(const KktPlan& P, const KktKnobs& knobs);

// One step of a substitution sweep: a kind and up to four integers.  The
// level kinds stand in both lists, for their forward kernel(s) in `fwd` and
// their backward kernel(s) in `bwd`; q0 indexes the sweep order.
enum SweepKind {
    kSwChunked = 0,   // k_fwd_diag + k_fwd_gemv / k_bwd_partial + k_bwd_finish: n supernodes from q0, b chunks from a
    kSwPlain,         // k_forward / k_backward: n supernodes from q0
    kSwLeaf8,         // k_fwd_leaf8 / k_bwd_leaf8: n small leaves from q0
    kSwMerged,        // k_fwd_level / k_bwd_level: n leaves from q0, then a other supernodes
    kSwLeaf,          // k_fwd_leaf / k_bwd_leaf: n leaves from q0
    kSwPre,           // k_fwd_pre: n columns (deep trees)
    kSwSyncFree,      // k_fwd_sf / k_bwd_sf: n items; a: the forward launch reads the late lists
    kSwTailGather,    // k_tail_gather, between tail_rhs_begin and tail_rhs_end
    kSwTailLead,      // k_tail_fwd_lead
    kSwTailChain,     // k_tail_fwd_chain / k_tail_bwd_chain
    kSwTailPair,      // k_tail_bwd_pair
    kSwTailBlock,     // k_tail_fwd / k_tail_bwd of block column a (blocked tails, one right-hand side)
    kSwTailDscale,    // k_tail_dscale (blocked tails)
};
struct SweepStep { int kind, q0, n, a, b; };
struct SweepSteps {
    std::vector<SweepStep> fwd, bwd;   // in launch order
    // Leading forward steps that read only the sparse panels and the
    // right-hand side: fwd[0, split) ends with the list's TailGather, and
    // fwd[split] is the TailLead.  KktDevice enqueues them beside the dense
    // tail's factorisation (the forward pre-pass, kkt_device.h).  0: no such
    // pair in the list (no tail, a blocked tail, the per-block chain).
    int split = 0;
    // The step after the TailLead: where a solve's first sweep starts when the
    // pre-pass also ran the lead, behind or beside the dense tail's factor
    // (IPO_HIP_LEAD_TRAIL, kkt_device.h).  Non-zero exactly when the list has
    // a TailLead.
    int lead_end = 0;
};
// the rule of SweepSteps::split, on any forward list
int sweep_split(const std::vector<SweepStep>& fwd);
// the rule of SweepSteps::lead_end
int sweep_lead_end(const std::vector<SweepStep>& fwd);
// kernel launches of a list: Chunked two, every other step one
int sweep_launches(const std::vector<SweepStep>& steps);

// What the launch code reads on the host: per-level and per-group pointers
// and counts, strides and flags.  Everything else a step builds is a local of
// that step, gone once uploaded.
struct KktLaunch {
    KktPaths paths;
    // panels
    std::vector<int> fu_ptr;         // per level: fused panel units [fu_ptr[l], fu_ptr[l+1])
    std::vector<int> small_ptr;      // per level: small panels [small_ptr[l], small_ptr[l+1]) (k_panel_s)
    std::vector<char> split_level;   // per level: k_diag + k_trsm instead of the fused panels (wide levels)
    std::vector<int> small1_cnt;     // per level: leading single-column small panels of <= 8 rows (k_panel_s1)
    // sweeps
    SweepSteps sweep;                // the launches of a substitution sweep (run_sweep_steps)
    size_t partial_stride = 1;       // backward partial sums of one right-hand side
    int sf_level = 0;                // first level of the sync-free range (nlevels: none)
    size_t ybuf_stride = 1, zpad_stride = 1;
    // gather groups (sparse level l, group nlevels = tail)
    std::vector<int> ck_ptr;         // per group: chunks [ck_ptr[g], ck_ptr[g+1])
    std::vector<int> ck_kind;        // per group: 0 k_update, 1 k_update_flat, 2 k_update_quad
    std::vector<char> ck_wide;       // per group: partials summed four at a time (few chunks, units split >= 4 ways)
    // dense tail
    std::vector<int> visit_ptr;      // TailView::vptr (empty: the visit_hi formula alone)
    std::vector<int> run_ptr;        // first item of each launch of the persistent run
};

// Fused panel units (k_panel_w) and small panels (k_panel_s) per level
struct PanelUnits {
    std::vector<int> fu_sup, fu_j;   // fused unit -> supernode, tile pair index
    std::vector<int> small_sups;
    std::vector<int> fu_ptr, small_ptr, small1_cnt;
    std::vector<char> split_level;
};
PanelUnits build_panel_units(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths);

// Solve chunks of the chunked levels
struct SolveChunks {
    std::vector<int> chunk_sup, chunk_r0;
    std::vector<int> sup_chunk0;     // per supernode: first solve chunk (-1: not chunked)
    std::vector<int> chunk_ptr;
    size_t partial_stride = 1;
};
SolveChunks build_solve_chunks(const KktPlan& P);

// level_sups in sweep order (leaves first on unchunked levels; a blocked
// tail's sweeps take no leaf kernels: the level order, counts zero)
struct SweepOrder {
    std::vector<int> sweep_sups;
    std::vector<int> leaf_cnt, leaf8_cnt;
};
SweepOrder build_sweep_order(const KktPlan& P, const KktPaths& paths, const SolveChunks& ch);

// Sync-free top levels of the sweeps (k_fwd_sf / k_bwd_sf)
struct SyncFreePlan {
    int sf_level = 0;
    std::vector<int> ybase;          // per supernode (+ end): first ybuf slot of its update values
    std::vector<int> yrow_idx;       // the plan's, through the moved slices
    std::vector<int> zbase, zpi, need, par;
    std::vector<SchedInt2> items_f, items_b;   // (s, -1) whole supernode, (s, c >= 0) solve chunk c
    size_t ybuf_stride = 1, zpad_stride = 1;
    // deep trees (paths.visits, a range exists): late lists and the pre-pass
    bool late_lists = false;
    std::vector<int> ylate_ptr, ylate_idx, pre_col, pre_ptr, pre_idx;
    bool range(const KktPlan& P) const { return sf_level < P.nlevels; }
};
SyncFreePlan build_sync_free_plan(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths,
                                  const SolveChunks& ch);

// Deep trees: the sparse units' k-slots in visit order (empty without visits)
struct VisitSlots {
    std::vector<int> kslot, kptr, late_b;        // the slots; per unit: its range's end, its first late slot
    std::vector<std::vector<SchedInt3>> vis;     // per gather group: (unit, slot begin, slot end)
};
VisitSlots build_visit_slots(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths);

// Split-K gather chunks per group
struct GatherChunks {
    std::vector<int> ck_u, ck_b, ck_e, ck_part;
    std::vector<int> ck_q;           // split-unit index of each chunk (-1: unsplit)
    std::vector<int> sp_u, sp_p0, sp_n;
    std::vector<int> ck_ptr, sp_ptr, ck_kind;
    std::vector<char> ck_wide;
    size_t split_cnt = 1;            // arrival counters of the split units
    size_t partial_tiles = 1;        // partial tiles of the largest group
};
GatherChunks build_gather_chunks(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths,
                                 const VisitSlots& vs);

// The launches of a substitution sweep.  Forward: levels [0, sf_level)
// ascending, each as one Chunked step or as Leaf8, then Merged or Leaf and
// Plain; Pre and SyncFree where a sync-free range exists; on a dense tail
// TailGather and TailLead or TailChain.  Backward: TailPair or TailChain,
// SyncFree, the levels descending, each level's steps in their forward order.
// blocked (paths.tail_blocked; an argument so that tests reach the rule on
// small plans): every level as Chunked or Plain, no Pre or SyncFree,
// TailGather and TailBlock 0 .. ntb - 1 forward, TailDscale and TailBlock
// ntb - 1 .. 0 at the head of the backward list.
SweepSteps build_sweep_steps(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths, const SolveChunks& ch,
                             const SweepOrder& order, const SyncFreePlan& sf, bool blocked);

// Launches per sweep (the step lists' totals) and algorithmic work per phase occurrence
struct WorkCounts {
    int fwd_launches = 0, bwd_launches = 0;
    double flops[kNumPhases] = {}, bytes[kNumPhases] = {};
};
WorkCounts count_work(const KktPlan& P, const KktKnobs& knobs, const SweepSteps& sweep);

// Per-task source descriptors and per-slot records of the gather
std::vector<TaskSrc> build_task_src(const KktPlan& P, const std::vector<TailTask>& ts);
std::vector<SlotRec> build_slot_records(const KktPlan& P, const std::vector<int>& kslot,
                                        const std::vector<TailTask>& ts);

// ---- the dense tail's host schedules

// Visits of launch t: block column c receives the updates of blocks 0 .. c - 2
// in chunks of K = TailView::vk, the latest chunk in launch c - 1, the one
// before in launch c - 2, ...: launch c - 1 - k applies blocks
// [c - 1 - K (k + 1), c - 1 - K k) (clipped at 0) -- every block available
// (b < t) and every column done before its panel, block c - 1 being the
// panel's own pre-update.  visit_hi: the end of the chunk launch t applies to
// column c (<= 0: none).
constexpr inline int visit_hi(int t, int c, int K) { return c - 1 - K * (c - 1 - t); }
// The count of TailRun::cdone[t] at which block column t of a tail of nt
// columns is readable while k_tail_run goes on (the trailing forward lead
// waits for it): every panel item of step t in tail_run_schedule signals once
// -- the step's panel workgroups, kkt_dense.hip tail_gp.
constexpr inline int lead_col_target(int nt, int t) {
    return (nt - t * kPanelCols + kTileRows - 1) / kTileRows - 1 > 1 ? (nt - t * kPanelCols + kTileRows - 1) / kTileRows - 1
                                                                      : 1;
}

// visit tiles of launch t (tail of ntb block columns, chunks of K blocks)
int tail_visit_tiles(int ntb, int t, int K);
// The visits of every look-ahead launch placed so that no launch needs more
// than `cap` workgroups (one round on `cap` CUs): visit_hi's chunks, with
// tiles' first chunks moved into earlier launches where a launch would
// overflow.  xcd: a column's visits grouped on one XCD within each launch.
// Returns the list (TailView::vlist layout) and ptr[0..ntb].
std::vector<unsigned> tail_visit_schedule(int ntb, int nt, int K, int cap, bool xcd, std::vector<int>& ptr);
// Items per launch t (ptr[t] .. ptr[t + 1]): panel workgroups (j, t | chunks
// of column t << 8 | 1 << 31), then visits (bi | c << 8 | b0 << 16 | b1 << 24,
// t | chunk index << 8), column t + 1's first.  Column c's chunks: the latest
// L blocks before c - 1 in launch c - 1, then K at a time in launches c - 2,
// ...; launches over `cap` items move first chunks earlier.
std::vector<SchedUint2> tail_run_schedule(int ntb, int nt, int K, int L, int cap, std::vector<int>& ptr);
// algorithmic flops / bytes of every visit of one factorisation
void tail_visit_work(int ntb, int nt, int K, double& flops, double& bytes);

// The schedules of the plan's dense tail (empty where a path is off)
struct TailSchedule {
    std::vector<unsigned> visit_list;     // TailView::vlist
    std::vector<int> visit_ptr;
    std::vector<SchedUint2> run_items;
    std::vector<int> run_ptr;
};
TailSchedule build_tail_schedule(const KktPlan& P, const KktKnobs& knobs, const KktPaths& paths, int cus);

// Every part, in the KktDevice constructor's order (tests and tools; the
// constructor calls the parts itself and drops each after its upload)
struct KktSchedule {
    KktPaths paths;
    PanelUnits panels;
    SolveChunks chunks;
    SweepOrder order;
    SyncFreePlan sf;
    VisitSlots visits;
    GatherChunks gather;
    SweepSteps sweep;
    WorkCounts work;
    std::vector<TaskSrc> usrc, tsrc;
    std::vector<SlotRec> slot_rec, tail_slot_rec;
    TailSchedule tail;
};
KktSchedule build_kkt_schedule(const KktPlan& P, const KktKnobs& knobs, int cus);

}  // namespace ipo
