// kkt_flags.h -- the factor pass's flag words (PlanView::flags, kkt_kernels.h),
// as the kernels write them and as the host reads them back.  Plain
// constants and a plain struct: host and device code alike include it.
#pragma once

namespace ipo {

// The words of PlanView::flags, one factor pass's verdict.  k_assemble_diag
// zeroes all of them; finish_pass reads the first kFlagReadWords back.
constexpr int kFlagNdep = 0;       // dependent pivots met so far (ldlt.c:600-614), summed by every factor kernel
constexpr int kFlagBail = 1;       // kBail* bits: fused kernels that stopped unwritten at a pivot failing the zero test
constexpr int kFlagTailBlock = 2;  // 1 + the first dense-tail block column whose look-ahead panel bailed (0: none);
                                   // the look-ahead's items poll it and skip themselves once it is set
constexpr int kFlagSpecNdep = 3;   // what the tail's last DEP pass added to kFlagNdep (k_tail_restore takes it back)
constexpr int kFlagWords = 4;
constexpr int kFlagReadWords = 3;  // kFlagNdep, kFlagBail, kFlagTailBlock
// kFlagBail: which kernel bailed (bit b counted in KktTimers::redo_where[b], b < 4)
constexpr int kBailRetired = 1;    // k_panel, which left; nothing sets it, redo_where[0] stays 0
constexpr int kBailSparse = 2;     // a fused sparse panel (k_panel_w / k_panel_ws): redo the factor per phase
constexpr int kBailTail = 4;       // a dense-tail look-ahead panel: repair from block column kFlagTailBlock - 1
constexpr int kBailSmall = 8;      // a small sparse panel (k_panel_s / k_panel_s1): redo the factor per phase
constexpr int kBailRestore = 16;   // with kBailTail: a DEP pass failed its check after other workgroups wrote,
                                   // so the repair restores the block column first (k_tail_restore)

// What finish_pass read back of one factor pass.  A sharded solve decides
// alike on every shard: *_all are the shards' maxima there, this device's
// own values otherwise.
struct FactorVerdict {
    double min_d = 0.0;     // min |d| over the factor (every shard's)
    int ndep = 0;           // kFlagNdep
    int bail = 0;           // kFlagBail: where this device's kernels bailed
    int tail_block = 0;     // kFlagTailBlock
    int ndep_all = 0, bail_all = 0;
    bool any_bail() const { return bail_all != 0; }
    // the look-ahead tail alone bailed: repairable from block column tail_col()
    bool tail_only() const { return (bail & ~kBailRestore) == kBailTail && tail_block > 0; }
    // ... after a DEP pass other workgroups of which wrote
    bool needs_restore() const { return (bail & kBailRestore) != 0; }
    int tail_col() const { return tail_block - 1; }
};

}  // namespace ipo
