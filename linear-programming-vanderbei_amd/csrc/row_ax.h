// row_ax.h -- A x by rows in column slices of x (host interface; the kernel
// is k_rows_ax_jds in dev_common.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "hip_util.h"
#include "kkt_knobs.h"

namespace ipo {

// A x by rows through jagged diagonals (bitwise sparse_dot's sums, see
// k_rows_ax_jds) when x exceeds kAxSliceBytes: KktKnobs::ax_blocks column
// slices, one pass each (default 1).  RowAxPlan holds A's
// entries by slice in jagged-diagonal order (built once, on the host, from
// the CSC of A); launch() writes ax[m], one kernel per pass.
constexpr long kAxSliceBytes = 2l << 20;
// whether A x goes through a RowAxPlan: KktKnobs::ax_jds when set, else more
// than one slice or x (n entries) larger than kAxSliceBytes
bool rows_ax_sliced(const KktKnobs& knobs, int n);
class RowAxPlan {
  public:
    void build(int m, int n, const int* kA, const int* iA, const double* A, int npass, hipStream_t st);
    void launch(const double* x, double* ax, hipStream_t st) const;
    // new values on the same pattern: dA (device) is A in build()'s CSC order
    void refresh(const double* dA, hipStream_t st);
    int passes() const { return np_; }

  private:
    int m_ = 0, np_ = 0, nz_ = 0;
    std::vector<int> rows_, nd_, dbase_;        // per pass: rows launched, diagonals, offset into dptr / dlen
    DevBuf<int> perm_, dptr_, dlen_, cols_;
    DevBuf<int> src_;                           // per slice position: its CSC entry (value_maps.h row_ax_layout)
    DevBuf<double> vals_;
};

}  // namespace ipo
