// value_maps.h -- where each value of a problem lives on the device, as index
// maps from the caller's arrays (host-only, pure functions: no HIP call), and
// the device refresh that reads them (value_refresh.hip).
//
// A context keeps one sparsity pattern; ipo_hip_ctx_update replaces the
// numbers on it.  Every derived copy of a value array is a gather of the
// caller's array through one of these maps:
//   CSR of A          at[d]   = A[csr[d]]            csr_value_map
//   RowAxPlan slices  vals[q] = A[src[q]]            row_ax_layout
//   Q's diagonal      qd[j]   = Q[qdiag[j]] or 0     q_diag_map
// and Q's symmetry is checked against q_transpose_map.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace ipo {

// map[d] = k: entry d of the CSR of A (m x n CSC kA / iA), in csc_transpose's
// order (lp_io.cpp: rows ascending, a row's entries in CSC order), is CSC
// entry k.  A permutation of [0, kA[n]).
std::vector<int> csr_value_map(int m, int n, const int* kA, const int* iA);

// A's entries by column slice in jagged-diagonal order (row_ax.h, k_rows_ax_jds):
// npass slices of ceil(n / npass) columns; per pass p the rows by entry count
// (descending, row order among equals) at perm[p m ..], rows[p] of them
// launched, nd[p] diagonals whose start / length stand at dptr / dlen[dbase[p]
// ..]; slice position q holds column cols[q] and CSC entry src[q].  src is a
// permutation of [0, kA[n]).
struct RowAxLayout {
    int np = 0;
    std::vector<int> rows, nd, dbase;
    std::vector<int> perm, dptr, dlen, cols, src;
};
RowAxLayout row_ax_layout(int m, int n, const int* kA, const int* iA, int npass);

// Q n x n CSC.  q_diag_map: [n], the entry (j, j) of column j, -1 without one.
// q_transpose_map: [kQ[n]], for entry k = (i, j) the entry (j, i); throws
// std::invalid_argument when the pattern has no such entry (not symmetric).
// Rows need not be sorted.  An involution that fixes the diagonal entries.
std::vector<int> q_diag_map(int n, const int* kQ, const int* iQ);
std::vector<int> q_transpose_map(int n, const int* kQ, const int* iQ);

// ---- the device side (value_refresh.hip) ----------------------------------
// dst[i] = map[i] >= 0 ? src[map[i]] : 0 for i < n (grid-stride; map and dst
// four entries at a time, 16 bytes wide, when both are 16-byte aligned)
void launch_gather_map(int n, const int* map, const double* src, double* dst, hipStream_t st);
// The validation reductions.  Each lowers *first (an int the caller set to
// INT_MAX) to the smallest offending index:
//   finite:    v[i] is NaN or +-Inf
//   positive:  !(v[i] > 0) or v[i] is not finite
//   symmetric: v[i] != v[tmap[i]]
void launch_first_nonfinite(int n, const double* v, int* first, hipStream_t st);
void launch_first_nonpositive(int n, const double* v, int* first, hipStream_t st);
void launch_first_asymmetric(int n, const double* v, const int* tmap, int* first, hipStream_t st);
// dst[j][i] = max(src[j][i], floor) for i < len[j], j < 4: one kernel
struct ClampJobs {
    const double* src[4];
    double* dst[4];
    int len[4];
};
void launch_clamp_copy4(const ClampJobs& J, double floor, hipStream_t st);

}  // namespace ipo
