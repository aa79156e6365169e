// kkt_knobs.h -- every environment variable the device code honours, read
// once into a KktKnobs when a KktDevice / IpmSolver is constructed.  This is
// the only place the .hip files' knobs touch the environment, and each
// member's comment is that knob's documentation (DESIGN.md "Runtime knobs"
// is the same list as a table, with the host-side variables of
// kkt_symbolic.cpp and capi.cpp).  A variable changed after an object is
// built does not reach that object.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <string>

#include "kkt_plan.h"

namespace ipo {

// Blocks per visit of the look-ahead dense tail (kkt_schedule.h, visit_hi).
// Measured on dfl001's tail (tools/ubench_tail): per-step launches (round 4)
// 4 -> 2.43 ms, 6 -> 2.26, 8 -> 2.55; the persistent run with the window
// hand-off (round 6, latest chunk L in brackets) 3 -> 1.92 (3), 4 -> 1.79
// (4), 5 -> 1.80 (2-4), 6 -> 1.85 (2), 7 -> 1.96, 8 -> 2.08
constexpr int kTailVisitBlocks = 4;
// the persistent tail's latest chunk per column (tail_run_schedule): it must
// finish within one step; equal to the chunk, every tile receives the
// per-step launches' chunks (bitwise them)
constexpr int kTailVisitLatest = 4;
// Entries from which a column of Q is summed by a wave (IPO_HIP_Q_LONG): the
// long-row threshold of A's linking rows (IpmSolver, kLongRow)
constexpr int kLongQCol = 256;
// Helper workgroups of the trailing forward lead beside k_tail_run
// (IPO_HIP_LEAD_HELPERS; measured: DESIGN.md 6.6)
constexpr int kTrailHelpers = 8;
// Block columns from which the trailing lead is on by default (IPO_HIP_LEAD_TRAIL unset)
constexpr int kTrailMinBlocks = 4;

struct KktKnobs {
    // ---- switches: the other setting is the same arithmetic in the same
    // ---- order (or, where said, the reference path), held by GPU tests

    // IPO_HIP_PANEL (default 1; 0 off): fused diagonal-block + panel kernels.
    // 0: per-phase kernels only (k_diag + k_trsm + k_tail_syrk, the
    // dependent-pivot path), the reference of the fused ones to rounding.
    // test_gpu_panel.py (panel kinds), test_gpu_tail_shapes.py (panel0), tools/factor_variants.py
    bool panel = true;
    // IPO_HIP_MERGE_LEVELS (default 1; 0 off): a level's leaves and other
    // supernodes in one sweep launch (k_fwd_level / k_bwd_level) and its
    // fused and small panels in one factor launch (k_panel_ws); 0: separate
    // launches, bitwise.  test_gpu_panel.py::test_merged_level_sweeps_bitwise
    bool merge_levels = true;
    // IPO_HIP_SF (default on; only 0 has an effect): the sync-free top levels
    // of the sweeps (k_fwd_sf / k_bwd_sf); 0: per-level launches, bitwise.
    // test_gpu_panel.py::test_sync_free_sweeps_bitwise
    bool sf = true;
    // IPO_HIP_OVERLAP (default 1; 0 off): run_hsd forms mu, residuals and
    // right-hand sides on a side stream beside the factorisation (never with
    // an Exchange); 0: the sequential iteration, bitwise.
    // test_gpu_panel.py::test_hsd_overlap_bitwise
    bool overlap = true;
    // IPO_HIP_PREPASS (default 1; 0 off): the overlapped HSD iteration has the
    // factorisation enqueue the first solve's maxbc, k_perm_in2 and forward
    // steps up to k_tail_gather on the side stream beside the dense tail's
    // factor (KktDevice::PrePass; fused panels, the persistent tail and the
    // lead sweep only); 0: the solve runs them itself, bitwise.  No gate on
    // the tail's block count: measured on one box, off against on alternated
    // (dfl001, 70 block columns: 292.9 -> 299.1 it/s; the others HSD solve
    // time in ms): greenbea (12) 252 -> 240; 25fv47 (7) 98.6 -> 90.7; nesm (6) 364 -> 352;
    // fffff800 (5) 74.7 -> 70.1; bnl1 (4) 94.1 -> 88.5; maros (4) 582 -> 569;
    // brandy (3) 26.4 -> 24.3; beaconfd (3) 20.3 -> 18.8; forplan, sctap3,
    // grow15 within their spread -- no tail small enough to lose.
    // test_gpu_prepass.py
    bool prepass = true;
    // IPO_HIP_LEAD_TRAIL (unset (-1): 2 for tails of at least kTrailMinBlocks
    // block columns, else 0; set: 0, 1 or 2, anything else as unset): where the
    // pre-pass is eligible, the factorisation also enqueues the first solve's
    // forward tail lead, in its trailing form (k_tail_fwd_lead<R, true>, which
    // reads a block column of the tail once k_tail_run's TailRun::cdone says
    // it is final and gives up if the run bails): 1 behind k_tail_run on its
    // stream, before the read-back (removes the host round trip between the
    // two); 2 beside it on the side stream, column by column.  The solve then
    // starts its first sweep after the lead (SweepSteps::lead_end); 0: the
    // solve runs the lead itself, after the read-back; bitwise.  Measured on
    // one box, alternated (dfl001, it/s, four runs each): parent 298.0-300.0,
    // 0: 299.3-300.9, 1: 296.3-298.3, 2: 309.1-312.2 -- 2 is the default, its
    // slowest run above the parent's fastest.  HSD solve time
    // in ms, parent against 2, medians of three processes of ten solves:
    // greenbea (12 block columns) 235.4 -> 232.4, 25fv47 (7) 90.2 -> 87.6,
    // nesm (6) 353.1 -> 353.4, bnl1 (4) 89.0 -> 87.3, brandy (3) 24.4 -> 24.6,
    // beaconfd (3) 18.8 -> 19.1: tails without a helper block (at most
    // kLeadBlocks + 1 = 3 block columns, a lead of ~10 us) gain nothing and
    // pay the extra event and launch, so the default leaves them alone.
    // test_gpu_lead_trail.py, test_lead_trail.py
    int lead_trail = -1;
    int lead_trail_mode(int ntb) const { return lead_trail >= 0 ? lead_trail : ntb >= kTrailMinBlocks ? 2 : 0; }
    // IPO_HIP_LEAD_HELPERS (default kTrailHelpers; max(1, v)): helper
    // workgroups of the trailing lead beside the run (mode 2), which take the
    // blocks by ticket.  Each holds the launch's dynamic LDS on a CU that then
    // has no room for a k_tail_run workgroup, so fewer cost the run less; too
    // few fall behind the lead (dfl001, 70 block columns, it/s against the
    // parent's 299: 8 310, 4 311, 2 269, 1 193).  Bitwise.
    int lead_helpers = kTrailHelpers;
    // IPO_HIP_CHAIN_LEAD (default on unless it parses to 0; dense tails of at
    // most kChainMaxBlocks block columns): the forward dense-tail sweep by one
    // lead workgroup + helpers (k_tail_fwd_lead); 0: the per-block chain,
    // bitwise.  test_gpu_panel.py, test_gpu_tail_shapes.py (lead0)
    bool chain_lead = true;
    // IPO_HIP_CHAIN_PAIRS (default off; on when it parses to non-zero): two
    // 64-row blocks per workgroup of the backward dense-tail chain
    // (k_tail_bwd_pair), bitwise.  test_gpu_panel.py, test_gpu_tail_shapes.py (pairs)
    bool chain_pairs = false;
    // IPO_HIP_TAIL_RUN (default on unless it parses to 0; tails of at most
    // kTailSchedMaxBlocks block columns): the look-ahead dense tail as one
    // persistent launch (k_tail_run); 0: one launch per step, bitwise at
    // VISIT_LATEST = VISIT_BLOCKS.  test_gpu_panel.py, test_gpu_tail_shapes.py (run0)
    bool tail_run = true;
    // IPO_HIP_TAIL_WINPUB (default on unless it parses to 0): each step's tile
    // windows handed to the next step's pre-update as they complete
    // (kkt_dense.hip RunPub); 0: the pre-update waits for the whole previous
    // step and reads S, bitwise.  test_gpu_panel.py, test_gpu_tail_shapes.py (winpub0)
    bool tail_winpub = true;
    // IPO_HIP_VISIT_SCHED (default on unless it parses to 0): look-ahead
    // launches of at most one workgroup per CU (tail_visit_schedule); 0: the
    // visit_hi formula alone, bitwise.  test_gpu_panel.py, test_gpu_tail_shapes.py
    // (sched0); tools/ubench_tail reads it itself
    bool visit_sched = true;
    // IPO_HIP_VISIT_XCD (default on unless it parses to 0): the schedule's
    // visits of one column on workgroup ids of one residue mod 8 (one XCD's
    // L2); order within a launch only, bitwise.  test_gpu_panel.py,
    // test_gpu_tail_shapes.py (xcd0)
    bool visit_xcd = true;
    // IPO_HIP_TAIL_REPAIR (default on unless it parses to 0): a dependent
    // pivot in the look-ahead tail redoes only the bailed block column and
    // resumes (never without the fused kernels or with an Exchange); 0: the
    // whole factorisation again by the per-phase kernels.  Use
    // KktDevice::tail_repair().  test_gpu_panel.py::test_tail_repair, tools/factor_variants.py
    bool tail_repair = true;
    // IPO_HIP_TAIL_SPEC (default 1; atoi): TailView::dep when the host repair
    // backs it -- dependent pivots inside the look-ahead panel (0: bail to
    // the host, 2: the tests' forced path).  test_gpu_panel.py
    int tail_spec = 1;
    // IPO_HIP_SPARSE_DEP (default 1; atoi): TailView::sdep -- dependent pivots
    // inside the sparse fused panels (0: redo the factor).  test_gpu_panel.py
    int sparse_dep = 1;
    // IPO_HIP_VISITS (unset: deep trees only, see deep_tree(); else on when
    // non-zero): the deep-tree gather schedule (early k-slots as visits in
    // lower levels' launches) and the sweeps' pre-pass (k_fwd_pre).
    // test_gpu_deep.py
    int visits = -1;
    // IPO_HIP_GATHER_FLAT (default 1; the integer 0/1/2): flat gathers
    // (k_update_flat) for latency-bound launches: 0 never, 1 deep trees,
    // 2 every launch of at most kFlatMaxChunks chunks; bitwise.  test_gpu_deep.py
    int gather_flat = 1;
    // IPO_HIP_GATHER_QUAD (default 1; 0 off): quadrant gathers (k_update_quad)
    // on the narrow levels of deep trees; 0: the flat gather, bitwise where it
    // splits no unit.  test_gpu_sparse_shapes.py (visits, visits_noquad)
    bool gather_quad = true;
    // IPO_HIP_SMALL_LEAVES (unset (-1): kSmallLeafMinCount, kkt_schedule.h;
    // else max(0, v); 0 never): levels with at least this many small leaves
    // sweep them eight to a wave (k_fwd_leaf8 / k_bwd_leaf8), and levels with
    // at least this many single-column small panels of <= 8 rows factor them
    // eight to a wave (k_panel_s1); bitwise.
    // test_gpu_panel.py::test_small_leaves_bitwise
    int small_leaves = -1;
    // IPO_HIP_PANEL_SPLIT (default 768; max(0, v); 0 never): the fused-unit
    // count from which a level of >= 4 units per supernode runs k_diag +
    // k_trsm instead; bitwise.  test_gpu_panel.py::test_split_panel_levels_bitwise
    int panel_split = 768;
    // IPO_HIP_AX_BLOCKS (default 1; max(1, v)): column slices of x, one pass
    // each, of the row products A x (RowAxPlan, row_ax.h); bitwise.  Measured
    // on BASELINE configs[3]'s uniform LP (x 8 MB): one pass 72.6 us per
    // residual launch, 2 / 3 / 4 / 8 slices 77.5 / 79.1 / 85 / 123 us (the
    // jagged-diagonal entry loads made the slices' locality worth less than
    // their extra passes), so large problems take one pass by default.
    // test_gpu_rowax.py
    int ax_blocks = 1;
    // IPO_HIP_AX_JDS (unset (-1): when x exceeds kAxSliceBytes or AX_BLOCKS >
    // 1; else on when non-zero): A x through a RowAxPlan (rows_ax_sliced)
    int ax_jds = -1;

    // ---- tuning values (results change to rounding at most)

    // IPO_HIP_VISIT_BLOCKS (default kTailVisitBlocks; max(1, v)): TailView::vk,
    // blocks per deferred trailing update of a dense-tail tile.
    // test_gpu_panel.py, test_gpu_tail_shapes.py (kl1, kl6); tools/ubench_tail reads it itself
    int visit_blocks = kTailVisitBlocks;
    // IPO_HIP_VISIT_LATEST (default kTailVisitLatest; max(1, v)): the
    // persistent tail's latest chunk per column, in blocks.
    // test_gpu_panel.py, test_gpu_tail_shapes.py
    int visit_latest = kTailVisitLatest;
    // IPO_HIP_VISIT_SLOTS (default kVisitSlots; max(1, v / kSlab) slabs):
    // k-slots per deep-tree visit, held here in slabs of kSlab.
    // test_gpu_sparse_shapes.py (vslots16)
    int visit_slabs = kVisitSlots / kSlab;
    // IPO_HIP_MIN_CHUNK (default 64; max(kSlab, v / kSlab * kSlab)): smallest
    // split-K gather chunk in k-slots; 64 measured best of 16-256 on
    // configs[3] and dfl001.  test_gpu_sparse_shapes.py (chunk16), tools/chunk_ab.py
    int min_chunk = 64;
    // IPO_HIP_SF_WIDTH (unset (-1): 300 for factors of fewer than 2^25
    // entries, 64 above; else max(1, v)): the sync-free range holds the top
    // levels of at most this many supernodes (kkt_paths, kkt_schedule.cpp);
    // bitwise.  test_gpu_sparse_shapes.py (sfw1)
    int sf_width = -1;
    // IPO_HIP_UPDATE_XCD (default 1024; max(0, v); 0 off): PlanView::xcd --
    // gather launches of at least this many chunks walk them XCD by XCD;
    // bitwise.  test_gpu_sparse_shapes.py (xcd1)
    int update_xcd = 1024;
    // IPO_HIP_UPDATE_OCC (default 4; atoi): 4: k_update<1, 4> (four
    // workgroups per CU), anything else k_update<1, 1>; bitwise.
    // test_gpu_sparse_shapes.py (occ1)
    int update_occ = 4;
    // IPO_HIP_DOT_SEGMIN (unset (-1): kSegDotLen for LPs with a vector of
    // kOrderedMaxLen entries, else 0; set: max(0, v)): RedJobs::segmin of the
    // solver's dots (dev_common.h)
    int dot_segmin = -1;
    // IPO_HIP_Q_LONG (unset: kLongQCol = 256; max(0, v); 0 never): columns of
    // Q with at least this many entries are summed by one wave each
    // (launch_q_long, dev_common.h: lanes strided, then a wave sum -- a fixed
    // order, not sparse_dot's) in the QP residual and the refinement's
    // residual; 0: one thread walks every column serially.  An empty column
    // is never long.  (The test entry ipo_hip_q_times, capi.cpp, reads it at
    // each call with long_min <= 0.)  test_gpu_qp_dense.py
    int q_long = kLongQCol;

    // ---- developer diagnostics

    // IPO_HIP_SETUP_TIMES (presence): KktDevice's setup steps timed to stderr
    bool setup_times = false;
    // IPO_HIP_DEBUG_REDO (presence): redo / repair counts to stderr when a
    // KktDevice is destroyed.  tools/redo_stats.py, tools/factor_variants.py, tools/trace_one.sh
    bool debug_redo = false;
    // IPO_HIP_TRACE_FULL (presence): full-precision scalars per HSD iteration
    // on stderr.  tools/gpu_dump.py, tools/status_loss_probe.py
    bool trace_full = false;
    // IPO_HIP_DUMP_DIR (a directory; unset or empty: off): every
    // factorisation's input and outcome to <dir>/fNNNN.bin (dump_factor).
    // tools/dep_compare.py, tools/gpu_dump.py, tools/tail_diag.py, tools/factor_variants.py
    std::string dump_dir;
    // IPO_HIP_GATHER_STAMPS (default -1: none; atoi): the gather group whose
    // first flat / quadrant launch prints its in-kernel stamps
    int gather_stamps = -1;
    // IPO_HIP_EPSDIAG_MAX (default 0: the reference's unbounded growth; atof):
    // a cap on eps_diag's x10 growth.  tools/status_loss_probe.py
    double epsdiag_max = 0.0;
    // IPO_HIP_PIVTOL (default 1e-17, see KktDevice::pivot_tol_; atof): the
    // zero-pivot tolerance a KktDevice starts with (set_pivot_tolerance
    // overrides).  tools/tau_sweep.py
    double pivtol = 1.0e-17;
    // IPO_SF_STAMPS_FILE (a file; -DIPO_SF_STAMPS builds only): the forward
    // sync-free sweep's per-item stamps.  tools/sf_critical.py
    std::string sf_stamps_file;

    // the deep-tree schedule of IPO_HIP_VISITS: forced, else from kVisitLevels levels up
    bool deep_tree(int nlevels) const { return visits < 0 ? nlevels >= kVisitLevels : visits != 0; }

    static KktKnobs from_env() {
        const auto flag = [](const char* name, bool dflt) {     // set: on unless it parses to 0
            const char* e = std::getenv(name);
            return e ? std::atoi(e) != 0 : dflt;
        };
        const auto num = [](const char* name, int dflt) {
            const char* e = std::getenv(name);
            return e ? std::atoi(e) : dflt;
        };
        const auto real = [](const char* name, double dflt) {
            const char* e = std::getenv(name);
            return e ? std::atof(e) : dflt;
        };
        const auto text = [](const char* name) {
            const char* e = std::getenv(name);
            return std::string(e ? e : "");
        };
        const auto set = [](const char* name) { return std::getenv(name) != nullptr; };
        KktKnobs k;
        k.panel = flag("IPO_HIP_PANEL", true);
        k.merge_levels = flag("IPO_HIP_MERGE_LEVELS", true);
        k.sf = flag("IPO_HIP_SF", true);
        k.overlap = flag("IPO_HIP_OVERLAP", true);
        k.prepass = flag("IPO_HIP_PREPASS", true);
        k.lead_trail = num("IPO_HIP_LEAD_TRAIL", -1);
        if (k.lead_trail < 0 || k.lead_trail > 2) k.lead_trail = -1;
        k.lead_helpers = std::max(1, num("IPO_HIP_LEAD_HELPERS", kTrailHelpers));
        k.chain_lead = flag("IPO_HIP_CHAIN_LEAD", true);
        k.chain_pairs = flag("IPO_HIP_CHAIN_PAIRS", false);
        k.tail_run = flag("IPO_HIP_TAIL_RUN", true);
        k.tail_winpub = flag("IPO_HIP_TAIL_WINPUB", true);
        k.visit_sched = flag("IPO_HIP_VISIT_SCHED", true);
        k.visit_xcd = flag("IPO_HIP_VISIT_XCD", true);
        k.tail_repair = flag("IPO_HIP_TAIL_REPAIR", true);
        k.tail_spec = num("IPO_HIP_TAIL_SPEC", 1);
        k.sparse_dep = num("IPO_HIP_SPARSE_DEP", 1);
        if (set("IPO_HIP_VISITS")) k.visits = flag("IPO_HIP_VISITS", false);
        k.gather_flat = num("IPO_HIP_GATHER_FLAT", 1);
        k.gather_quad = flag("IPO_HIP_GATHER_QUAD", true);
        if (set("IPO_HIP_SMALL_LEAVES")) k.small_leaves = std::max(0, num("IPO_HIP_SMALL_LEAVES", 0));
        k.panel_split = std::max(0, num("IPO_HIP_PANEL_SPLIT", 768));
        k.ax_blocks = std::max(1, num("IPO_HIP_AX_BLOCKS", 1));
        if (set("IPO_HIP_AX_JDS")) k.ax_jds = flag("IPO_HIP_AX_JDS", false);
        k.visit_blocks = std::max(1, num("IPO_HIP_VISIT_BLOCKS", kTailVisitBlocks));
        k.visit_latest = std::max(1, num("IPO_HIP_VISIT_LATEST", kTailVisitLatest));
        if (set("IPO_HIP_VISIT_SLOTS")) k.visit_slabs = std::max(1, num("IPO_HIP_VISIT_SLOTS", 0) / kSlab);
        if (set("IPO_HIP_MIN_CHUNK")) k.min_chunk = std::max(kSlab, num("IPO_HIP_MIN_CHUNK", 0) / kSlab * kSlab);
        if (set("IPO_HIP_SF_WIDTH")) k.sf_width = std::max(1, num("IPO_HIP_SF_WIDTH", 0));
        k.update_xcd = std::max(0, num("IPO_HIP_UPDATE_XCD", 1024));
        k.update_occ = num("IPO_HIP_UPDATE_OCC", 4);
        if (set("IPO_HIP_DOT_SEGMIN")) k.dot_segmin = std::max(0, num("IPO_HIP_DOT_SEGMIN", 0));
        k.q_long = std::max(0, num("IPO_HIP_Q_LONG", kLongQCol));
        k.setup_times = set("IPO_HIP_SETUP_TIMES");
        k.debug_redo = set("IPO_HIP_DEBUG_REDO");
        k.trace_full = set("IPO_HIP_TRACE_FULL");
        k.dump_dir = text("IPO_HIP_DUMP_DIR");
        k.gather_stamps = num("IPO_HIP_GATHER_STAMPS", -1);
        k.epsdiag_max = real("IPO_HIP_EPSDIAG_MAX", 0.0);
        k.pivtol = real("IPO_HIP_PIVTOL", 1.0e-17);
        k.sf_stamps_file = text("IPO_SF_STAMPS_FILE");
        return k;
    }
};

}  // namespace ipo
