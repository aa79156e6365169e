// value_maps.cpp -- the index maps of value_maps.h (host-only, no HIP call).
#include "value_maps.h"

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace ipo {

std::vector<int> csr_value_map(int m, int n, const int* kA, const int* iA) {
    const int nz = kA[n];
    std::vector<int> fill(m + 1, 0), map(nz);
    for (int k = 0; k < nz; k++) fill[iA[k] + 1]++;
    for (int i = 0; i < m; i++) fill[i + 1] += fill[i];
    for (int k = 0; k < nz; k++) map[fill[iA[k]]++] = k;
    return map;
}

RowAxLayout row_ax_layout(int m, int n, const int* kA, const int* iA, int npass) {
    RowAxLayout L;
    const int np = L.np = std::max(1, npass);
    const int per = (n + np - 1) / np;
    auto slice = [&](int j) { return per > 0 ? std::min(np - 1, j / per) : 0; };
    // entries per (pass, row), the rows of each pass by count (descending,
    // row order among equal counts), the diagonals
    std::vector<int> cnt(static_cast<size_t>(np) * m, 0);
    for (int j = 0; j < n; j++)
        for (int k = kA[j]; k < kA[j + 1]; k++) cnt[static_cast<size_t>(slice(j)) * m + iA[k]]++;
    std::vector<int> rank(static_cast<size_t>(np) * m);
    L.perm.resize(static_cast<size_t>(np) * m);
    L.rows.assign(np, 0);
    L.nd.assign(np, 0);
    L.dbase.assign(np + 1, 0);
    long nz = 0;
    for (int p = 0; p < np; p++) {
        const int* c = cnt.data() + static_cast<size_t>(p) * m;
        int mx = 0;
        for (int i = 0; i < m; i++) mx = std::max(mx, c[i]);
        std::vector<int> bucket(mx + 2, 0);          // rows with count >= v start at bucket[mx - v]
        for (int i = 0; i < m; i++) bucket[mx - c[i] + 1]++;
        for (int v = 0; v <= mx; v++) bucket[v + 1] += bucket[v];
        int* pp = L.perm.data() + static_cast<size_t>(p) * m;
        int* rk = rank.data() + static_cast<size_t>(p) * m;
        for (int i = 0; i < m; i++) { const int r = bucket[mx - c[i]]++; pp[r] = i; rk[i] = r; }
        // pass 0 writes every row (a row with no entry in it gets 0); later
        // passes only the rows that have entries in their slice
        int active = 0;
        while (active < m && c[pp[active]] > 0) active++;
        L.rows[p] = p == 0 ? m : active;
        L.nd[p] = mx;
        for (int k = 0, len = active; k < mx; k++) {
            while (len > 0 && c[pp[len - 1]] <= k) len--;
            L.dptr.push_back(static_cast<int>(nz));
            L.dlen.push_back(len);
            nz += len;
        }
        L.dbase[p + 1] = static_cast<int>(L.dptr.size());
    }
    if (nz > static_cast<long>(INT32_MAX)) throw std::length_error("row products: more than 2^31 entries");
    L.cols.resize(nz);
    L.src.resize(nz);
    std::vector<int> fill(static_cast<size_t>(np) * m, 0);
    for (int j = 0; j < n; j++) {
        const int p = slice(j);
        for (int k = kA[j]; k < kA[j + 1]; k++) {
            const size_t pi = static_cast<size_t>(p) * m + iA[k];
            const int q = L.dptr[L.dbase[p] + fill[pi]++] + rank[pi];
            L.cols[q] = j;
            L.src[q] = k;
        }
    }
    return L;
}

std::vector<int> q_diag_map(int n, const int* kQ, const int* iQ) {
    std::vector<int> d(n > 0 ? n : 0, -1);
    for (int j = 0; j < n; j++)
        for (int k = kQ[j]; k < kQ[j + 1]; k++)
            if (iQ[k] == j) d[j] = k;      // the last one, as the diagonal's upload takes it
    return d;
}

std::vector<int> q_transpose_map(int n, const int* kQ, const int* iQ) {
    const int nz = n > 0 ? kQ[n] : 0;
    {
        // Rows ascending in every column (the layout a context accepts) and
        // the pattern symmetric: walking the columns in order, the entry
        // (j, i) is the next one of column i not yet paired -- one pass.
        std::vector<int> next(kQ, kQ + (n > 0 ? n : 0)), t(nz);
        bool ok = true;
        for (int j = 0; j < n && ok; j++)
            for (int k = kQ[j]; k < kQ[j + 1]; k++) {
                const int i = iQ[k], pos = next[i];
                if (pos >= kQ[i + 1] || iQ[pos] != j) { ok = false; break; }
                t[k] = pos;
                next[i] = pos + 1;
            }
        if (ok) return t;
    }
    // any row order: the CSR of Q's pattern: row i's entries by column, each with its CSC index
    const std::vector<int> csr = csr_value_map(n, n, kQ, iQ);
    std::vector<int> rptr(n + 1, 0), col(nz);
    for (int k = 0; k < nz; k++) rptr[iQ[k] + 1]++;
    for (int i = 0; i < n; i++) rptr[i + 1] += rptr[i];
    for (int j = 0; j < n; j++)
        for (int k = kQ[j]; k < kQ[j + 1]; k++) col[k] = j;
    // entry k = (i, j) pairs with the entry (j, i): in row j of the CSR, the one of column i
    std::vector<int> t(nz, -1);
    for (int j = 0; j < n; j++)
        for (int k = kQ[j]; k < kQ[j + 1]; k++) {
            const int i = iQ[k];
            // row j's entries have ascending columns: find column i
            const int* b = csr.data() + rptr[j];
            const int* e = csr.data() + rptr[j + 1];
            const int* f = std::lower_bound(b, e, i, [&](int kk, int want) { return col[kk] < want; });
            if (f == e || col[*f] != i)
                throw std::invalid_argument("Q: pattern not symmetric at (" + std::to_string(i) + ", " +
                                            std::to_string(j) + ")");
            t[k] = *f;
        }
    return t;
}

}  // namespace ipo
