// kkt_device.hip -- supernodal LDL^T of the quasi-definite KKT matrix on
// gfx950 (see kkt_device.h for the reference mapping).
//
// Data layout in HBM
//   Lx    supernode panels, column-major, panel s = h_s x nc_s (ld = h_s):
//         rows 0..nc-1 are the diagonal block (unit lower L11 after the
//         factor, diagonal slots hold K's diagonal on input), rows nc..h-1
//         are the rows R_s of L21.  One contiguous array, 8-B aligned.
//   dg    D of L D L' (new index order), live = the reference's mark[].
//
// This unit holds the factor and the refined solve:
//   assembly  of K(E, D) into Lx (k_assemble_*), the dense tail's clear.
//   gathers   per elimination-tree level and for the dense tail: the
//             left-looking split-K gather of every descendant panel's update
//             (k_update*, fixed slot order -> bitwise reproducible), and
//             k_tail_syrk, the per-phase path's trailing update.
//   KktDevice the constructor and its steps, factor* with the level and
//             tail launches (the dense per-panel kernels: kkt_dense.hip),
//             the tail repair, the phase timers, and solve_multi -- the
//             refinement loop of ldlt.c:367-416 with its permutation,
//             residual and copy kernels.
// The substitution sweeps (rawsolve: kernels and launches) are kkt_sweep.hip.
#include <hip/hip_runtime.h>

#include <chrono>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dev_common.h"
#include "kkt_device.h"
#include "kkt_kernels.h"
#include "lp_io.h"
#include "value_maps.h"

namespace ipo {

namespace {

// ---------------------------------------------------------------- assembly
__global__ void __launch_bounds__(NT)
k_assemble_A(int nz, const double* __restrict__ A, const int64_t* __restrict__ amap, double* __restrict__ Lx) {
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k < nz) Lx[amap[k]] = A[k];
}

// -max Q below the diagonal (ldlt.c:253-256: the entry whose new row is below
// its new column; its symmetric twin and the diagonal have qmap < 0)
__global__ void __launch_bounds__(NT)
k_assemble_Q(int nq, const double* __restrict__ Q, const int64_t* __restrict__ qmap, double qmax,
             double* __restrict__ Lx) {
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k < nq && qmap[k] >= 0) Lx[qmap[k]] = -qmax * Q[k];
}

// K's diagonal: -max(E, eps) on y-nodes, +max(D, eps) on x-nodes (ldlt.c:235-236),
// then -max Q_jj on the y-nodes of a Q block (ldlt.c:256); |terms| of each
__global__ void __launch_bounds__(NT)
k_assemble_diag(int T, int m, const int* __restrict__ perm, const double* __restrict__ E,
                const double* __restrict__ D, double eps, const int64_t* __restrict__ dslot,
                double* __restrict__ Lx, int* __restrict__ live, double* __restrict__ dscale, int tail_from,
                int* __restrict__ flags, const double* __restrict__ qdiag, double qmax) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v < kFlagWords) flags[v] = 0;      // the factorisation's flags (no fill launch of their own)
    if (v >= T) return;
    const int old = perm[v];
    // columns >= tail_from: replicated linking rows of a non-leading shard,
    // whose diagonal enters the summed tail once (from shard 0)
    double a = v >= tail_from ? 0.0 : old < m ? -ref_max(E[old], eps) : ref_max(D[old - m], eps);
    double sc = fabs(a);
    if (qdiag && old < m) {
        const double q = qmax * qdiag[old];
        a = a - q;
        sc = sc + fabs(q);
    }
    Lx[dslot[v]] = a;
    dscale[v] = sc;
    live[v] = 1;
}

// The dense tail's lower block triangle zeroed (column c from the first row
// of its diagonal block on): nothing reads the tail above its diagonal
// blocks (gathers, visits and panels write tiles bi >= bj, the sweeps read
// those and the diagonal blocks' upper slots), so the factorisation's clear
// skips that half of the nt x nt block.  One workgroup per column.
__global__ void __launch_bounds__(NT) k_zero_tail_lower(double* __restrict__ S, int nt) {
    const int c = blockIdx.x;
    double* col = S + (size_t)c * nt;
    for (int r = (c / kPanelCols) * kPanelCols + static_cast<int>(threadIdx.x); r < nt; r += NT) col[r] = 0.0;
}

// ------------------------------------------------------- left-looking gather
// out(r, c) -= sum_tasks sum_k L(row, k) * (d_k * L(col, k))     (ldlt.c:572,583)
// for one 64-row x (<= 64)-column output tile.  The inner dimension is the
// concatenation of every task's source columns (the plan's k-slot list);
// kSlab slots at a time are staged in LDS as A(r, k) = L(row(r), k) and
// B(c, k) = d_k L(col(c), k) -- zero where a task's row / column masks
// (TailTask) leave the tile entry untouched -- and multiplied with
// v_mfma_f64_16x16x4_f64, each of the 4 waves owning a 32x32 quarter.
// Slabs are double-buffered: the global loads of slab s+1 are in flight
// while slab s is multiplied.  The fixed slot order makes the sum bitwise
// reproducible.  Entries above the diagonal ((row0 + r) < (col0 + c)) are
// not written; on the diagonal the |terms| are added to dscale.
typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int KS = kSlab;

// What a k-slot needs (SlotRec, kkt_plan.h: masks, the source column's
// first row-set entry for the tile's rows, the column offset, d_k's index),
// expanded per slot on the host so that one coalesced load per slot stages a
// chunk's records in LDS; the values are then issued without a dependent
// metadata round trip.  ra = L(row, k), rb = d_k * L(col, k) (the reference
// form, ldlt.c:572,583), zero where the task leaves the tile entry untouched.
// The loads are unconditional (an unmarked lane reads the slot's first
// entry) and the mask / d_k product are applied after them (slot_fin): a
// load under a lane branch whose result the branch itself consumes makes
// the compiler wait for it before the branch joins -- one memory round trip
// per slot, measured as ~0.45 us per slot and wave (IPO_HIP_GATHER_STAMPS).
struct SlotLd {
    double a, b, d;
    bool ra, rb;
};
__device__ __forceinline__ SlotLd slot_ld(const SlotRec& m, const double* __restrict__ Lx,
                                          const double* __restrict__ dg, int lane) {
    const uint64_t below = (1ull << lane) - 1ull;
    SlotLd v;
    v.ra = (m.rmask >> lane) & 1ull;
    v.rb = (m.cmask >> lane) & 1ull;
    v.a = Lx[v.ra ? m.roff + __popcll(m.rmask & below) : m.roff];
    v.b = Lx[v.rb ? m.roff + m.cdelta + __popcll(m.cmask & below) : m.roff];
    v.d = dg[m.dk];
    return v;
}
__device__ __forceinline__ void slot_fin(const SlotLd& v, double& ra, double& rb) {
    ra = v.ra ? v.a : 0.0;
    rb = v.rb ? v.d * v.b : 0.0;
}

// Output tile of one gather unit: a 64-row tile of a sparse panel
// (tail < 0) or tile `tail` of the dense tail.
struct GatherTile {
    double* out;
    size_t ld;
    int nrow, ncol, row0, col0;
    double* dscale_col;      // non-null on tiles that hold diagonal entries
};

__device__ __forceinline__ GatherTile unit_tile(const PlanView& p, const TailView& tv, int u, int tail) {
    GatherTile g;
    if (tail < 0) {
        const int s = p.unit_sup[u], t = p.unit_tile[u];
        const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
        const int h = nc + (p.rowptr[s + 1] - p.rowptr[s]);
        const int rbase = t * TR;
        g.out = p.Lx + p.off[s] + rbase;
        g.ld = h;
        g.nrow = min(TR, h - rbase);
        g.ncol = nc;
        g.row0 = rbase;
        g.col0 = 0;
        g.dscale_col = t == 0 ? p.dscale + c0 : nullptr;
    } else {
        int bi = 0;
        while ((bi + 1) * (bi + 2) / 2 <= u) bi++;
        const int bj = u - bi * (bi + 1) / 2;
        g.out = tv.S + bi * TR + (size_t)(bj * TR) * tv.nt;
        g.ld = tv.nt;
        g.nrow = min(TR, tv.nt - bi * TR);
        g.ncol = min(TR, tv.nt - bj * TR);
        g.row0 = bi * TR;
        g.col0 = bj * TR;
        g.dscale_col = bi == bj ? p.dscale + tv.tc + bj * TR : nullptr;
    }
    return g;
}

// MFMA accumulation of slots [kb, ke) into this thread's 16 tile entries
// (acc[a][b][i] = entry (wr + 16a + (lane>>4) + 4i, wc + 16b + (lane&15)))
// and, for lanes on a diagonal entry, the |terms| of that entry (dabs).
// Pipeline: the slot values of slab sb + 1 are issued while slab sb is
// multiplied, the wave-uniform records of the slab after that one step
// ahead of its values (scalar loads, no LDS), LDS double-buffered.  (Deeper
// register rings, fragment skipping and a 4-waves-per-SIMD build were
// measured slower in round 2 and are gone: DESIGN.md section 6.)
__device__ void gather_acc(const PlanView& p, const SlotRec* __restrict__ recs, int kb, int ke, int dcol,
                           bool has_diag, double4_t (&acc)[2][2], double& dabs) {
    __shared__ double As[2][TR][KS + 1];
    __shared__ double Bs[2][TR][KS + 1];
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    dabs = 0.0;
    const int nk = ke - kb, nslab = nk / KS;
    double ra[KS / 4], rb[KS / 4];
    const double* __restrict__ Lx = p.Lx;
    const double* __restrict__ dg = p.dg;
    const SlotRec* __restrict__ wrec = recs + kb + wv * (KS / 4);
    SlotRec mn[KS / 4];
    auto fetch = [&](int slab) {
#pragma unroll
        for (int j = 0; j < KS / 4; j++) mn[j] = wrec[slab * KS + j];
    };
    auto issue = [&]() {
        SlotLd v[KS / 4];
#pragma unroll
        for (int j = 0; j < KS / 4; j++) v[j] = slot_ld(mn[j], Lx, dg, lane);
#pragma unroll
        for (int j = 0; j < KS / 4; j++) slot_fin(v[j], ra[j], rb[j]);
    };
    if (nslab > 0) { fetch(0); issue(); }
    if (1 < nslab) fetch(1);
#pragma unroll
    for (int j = 0; j < KS / 4; j++) { As[0][lane][wv * (KS / 4) + j] = ra[j]; Bs[0][lane][wv * (KS / 4) + j] = rb[j]; }
    __syncthreads();
    for (int sb = 0; sb < nslab; sb++) {
        const int cur = sb & 1;
        if (sb + 1 < nslab) {
            issue();
            if (sb + 2 < nslab) fetch(sb + 2);
        }
#pragma unroll
        for (int kk = 0; kk < KS; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; a++) av[a] = As[cur][wr + a * 16 + li][kk + lk];
#pragma unroll
            for (int b = 0; b < 2; b++) bv[b] = Bs[cur][wc + b * 16 + li][kk + lk];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        if (has_diag) {
#pragma unroll
            for (int j = 0; j < KS / 4; j++) {
                const int k = wv * (KS / 4) + j;
                dabs += fabs(As[cur][lane][k] * Bs[cur][dcol][k]);
            }
        }
        if (sb + 1 < nslab) {
#pragma unroll
            for (int j = 0; j < KS / 4; j++) {
                As[cur ^ 1][lane][wv * (KS / 4) + j] = ra[j];
                Bs[cur ^ 1][lane][wv * (KS / 4) + j] = rb[j];
            }
        }
        __syncthreads();
    }
}

// The tile's current values (read before the first store: the compiler
// cannot tell that the 16 entries are distinct and would otherwise
// serialise 16 round trips)
__device__ __forceinline__ void gather_old(const GatherTile& g, double (&old)[2][2][4]) {
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int rr = wr + a * 16 + (lane >> 4) + 4 * i;
                const int cc = wc + b * 16 + (lane & 15);
                const bool ok = rr < g.nrow && cc < g.ncol && g.row0 + rr >= g.col0 + cc;
                old[a][b][i] = ok ? g.out[rr + (size_t)cc * g.ld] : 0.0;
            }
}

// out = old - acc on the tile's lower part; dscale += the four waves' dabs in order
__device__ void gather_put(const GatherTile& g, const double (&old)[2][2][4], const double4_t (&acc)[2][2], double dabs,
                           bool has_diag, int dcol) {
    __shared__ double dred[4][TR];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int rr = wr + a * 16 + (lane >> 4) + 4 * i;
                const int cc = wc + b * 16 + (lane & 15);
                if (rr >= g.nrow || cc >= g.ncol || g.row0 + rr < g.col0 + cc) continue;
                g.out[rr + (size_t)cc * g.ld] = old[a][b][i] - acc[a][b][i];
            }
    if (g.dscale_col) {
        dred[wv][lane] = dabs;
        __syncthreads();
        if (wv == 0 && has_diag) g.dscale_col[dcol] += ((dred[0][lane] + dred[1][lane]) + dred[2][lane]) + dred[3][lane];
    }
}

__device__ __forceinline__ void gather_store(const GatherTile& g, const double4_t (&acc)[2][2], double dabs, bool has_diag,
                                             int dcol) {
    double old[2][2][4];
    gather_old(g, old);
    gather_put(g, old, acc, dabs, has_diag, dcol);
}

// Sum the np partial tiles of a split unit (slots p0.., thread-fragment
// order) in chunk order: acc = ((0 + P_0) + P_1) + ...  The partials were
// handed off inside this launch (sc1 loads, bypassing the CU's L1).
template <int SG>
__device__ __forceinline__ void split_sum(const double* __restrict__ partial, int p0, int np, double4_t (&acc)[2][2],
                                          double& dabs) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    dabs = 0.0;
    // SG partials' loads in flight at once (each a dependent round trip
    // otherwise: 12 partials took 12 of them), added in chunk order
    for (int j0 = 0; j0 < np; j0 += SG) {
        double v[SG][17];
#pragma unroll
        for (int g = 0; g < SG; g++) {
            const double* src = partial + (size_t)(p0 + min(j0 + g, np - 1)) * (TR * TR + 4 * TR);
#pragma unroll
            for (int e = 0; e < 16; e++) v[g][e] = sc1_load(src + e * NT + tid);
            v[g][16] = sc1_load(src + TR * TR + tid);
        }
#pragma unroll
        for (int g = 0; g < SG; g++) {
            if (j0 + g >= np) break;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int i = 0; i < 4; i++) acc[a][b][i] += v[g][(a * 2 + b) * 4 + i];
            dabs += v[g][16];
        }
    }
}

// Gather chunks: chunk c covers slots [ck_b[c], ck_e[c]) of unit ck_u[c].
// ck_part[c] < 0: the unit's only chunk, subtract directly.  Else the chunks
// of split unit q = ck_q[c] store their partial tiles (thread-fragment
// order) and dabs write-through (sc1) at partial slot ck_part[c], drain them,
// and one lane adds to the unit's arrival counter; the chunk whose add comes
// last sums all partials in chunk order (sc1 loads) and stores the tile
// (MI355X_MICROARCH.md hand-off table row 1: last arriver told by its own
// add's return value).  It resets the counter for the next factorisation.
// tail >= 0: units are dense-tail tiles.
// OCC: workgroups per CU the registers are sized for (1: the compiler's
// choice, 160 VGPRs = 3 per CU; 4 (default for SG = 1): 116 VGPRs, no
// spills -- one more workgroup's slab loads in flight per CU: dfl001's
// gather 51.1 -> 47.9 ms per solve, configs[3] / [4] +3 / +7 %;
// IPO_HIP_UPDATE_OCC=1 restores the compiler's choice)
template <int SG, int OCC>
__global__ void __launch_bounds__(NT, OCC)
k_update(PlanView p, TailView tv, int tail, const SlotRec* __restrict__ recs,
         const int* __restrict__ ck_u, const int* __restrict__ ck_b, const int* __restrict__ ck_e,
         const int* __restrict__ ck_part, int c0, double* __restrict__ partial,
         const int* __restrict__ ck_q, const int* __restrict__ sp_p0, const int* __restrict__ sp_n,
         int* __restrict__ split_cnt) {
    const int c = c0 + (p.xcd > 0 && static_cast<int>(gridDim.x) >= p.xcd ? xcd_chunk(blockIdx.x, gridDim.x)
                                                                     : static_cast<int>(blockIdx.x));
    const int u = ck_u[c], kb = ck_b[c], ke = ck_e[c], pi = ck_part[c];
    const GatherTile g = unit_tile(p, tv, u, tail);
    const int lane = threadIdx.x & 63;
    const int dcol = g.row0 + lane - g.col0;
    const bool has_diag = g.dscale_col && dcol >= 0 && dcol < g.ncol && lane < g.nrow;
    double4_t acc[2][2];
    double dabs;
    gather_acc(p, recs, kb, ke, dcol, has_diag, acc, dabs);
    if (pi < 0) {
        gather_store(g, acc, dabs, has_diag, dcol);
        return;
    }
    double* dst = partial + (size_t)pi * (TR * TR + 4 * TR);
    const int tid = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++) sc1_store(dst + ((a * 2 + b) * 4 + i) * NT + tid, acc[a][b][i]);
    sc1_store(dst + TR * TR + tid, dabs);
    __shared__ int last;
    const int q = ck_q[c];
    const int np = sp_n[q];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int prev = __hip_atomic_fetch_add(split_cnt + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = prev == np - 1;
        if (prev == np - 1) __hip_atomic_store(split_cnt + q, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    split_sum<SG>(partial, sp_p0[q], np, acc, dabs);
    gather_store(g, acc, dabs, has_diag, dcol);
}

// Flat gather for latency-bound launches (the level chain of deep trees,
// where a launch holds one small gather per unit and nothing hides the
// pipelined form's memory round trip per 16-slot slab -- 2.5 us each,
// measured): up to 64 slots per round, their records staged in LDS by one
// coalesced load, then every value of the round issued at once (32 loads
// in flight per lane), one barrier, the MFMA steps.  Slot k of a round is
// staged by the wave gather_acc gives it (k mod 16 in [4 wv, 4 wv + 4)) and
// the MFMA steps and |terms| run in gather_acc's order: bitwise the same.
constexpr int FK = 64;
#define GST(k) do { if (st && threadIdx.x == 0) st[k] = __builtin_amdgcn_s_memrealtime(); } while (0)
__device__ void gather_acc_flat(const PlanView& p, const SlotRec* __restrict__ recs, int kb, int ke, int dcol,
                                bool has_diag, double4_t (&acc)[2][2], double& dabs, long long* st = nullptr) {
    __shared__ double As[TR][FK + 1];
    __shared__ double Bs[TR][FK + 1];
    __shared__ SlotRec rl[FK];
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    dabs = 0.0;
    for (int k0 = kb; k0 < ke; k0 += FK) {
        const int nk = min(FK, ke - k0), nsl = nk / KS;
        if (tid < nk * 4)
            reinterpret_cast<uint64_t*>(rl)[tid] = reinterpret_cast<const uint64_t*>(recs + k0)[tid];
        __syncthreads();
        if (k0 == kb) GST(1);
        double ra[FK / 16 * 4], rb[FK / 16 * 4];
        SlotLd v[FK / 16 * 4];
#pragma unroll
        for (int sb = 0; sb < FK / KS; sb++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (sb < nsl) v[sb * 4 + j] = slot_ld(rl[sb * KS + wv * 4 + j], p.Lx, p.dg, lane);
#pragma unroll
        for (int sb = 0; sb < FK / KS; sb++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                ra[sb * 4 + j] = 0.0;
                rb[sb * 4 + j] = 0.0;
                if (sb < nsl) slot_fin(v[sb * 4 + j], ra[sb * 4 + j], rb[sb * 4 + j]);
            }
#pragma unroll
        for (int sb = 0; sb < FK / KS; sb++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (sb < nsl) {
                    As[lane][sb * KS + wv * 4 + j] = ra[sb * 4 + j];
                    Bs[lane][sb * KS + wv * 4 + j] = rb[sb * 4 + j];
                }
        __syncthreads();
        if (k0 == kb) GST(2);
        for (int kk = 0; kk < nk; kk += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int a = 0; a < 2; a++) av[a] = As[wr + a * 16 + li][kk + lk];
#pragma unroll
            for (int b = 0; b < 2; b++) bv[b] = Bs[wc + b * 16 + li][kk + lk];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
                    acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        if (has_diag) {
            for (int sb = 0; sb < nsl; sb++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int k = sb * KS + wv * 4 + j;
                    dabs += fabs(As[lane][k] * Bs[dcol][k]);
                }
        }
        __syncthreads();
        if (k0 == kb) GST(3);
    }
}

// k_update with the flat gather; an unsplit chunk reads its tile's old
// values before the gather (no workgroup writes a tile its launch reads:
// one chunk per unsplit unit, split units stored by their last chunk only)
template <int SG>
__global__ void __launch_bounds__(NT)
k_update_flat(PlanView p, TailView tv, int tail, const SlotRec* __restrict__ recs,
              const int* __restrict__ ck_u, const int* __restrict__ ck_b, const int* __restrict__ ck_e,
              const int* __restrict__ ck_part, int c0, double* __restrict__ partial,
              const int* __restrict__ ck_q, const int* __restrict__ sp_p0, const int* __restrict__ sp_n,
              int* __restrict__ split_cnt, long long* __restrict__ stamps) {
    long long* st = stamps && blockIdx.x < 1024 ? stamps + blockIdx.x * 8 : nullptr;
    GST(0);
    const int c = c0 + blockIdx.x;
    const int u = ck_u[c], kb = ck_b[c], ke = ck_e[c], pi = ck_part[c];
    const GatherTile g = unit_tile(p, tv, u, tail);
    const int lane = threadIdx.x & 63;
    const int dcol = g.row0 + lane - g.col0;
    const bool has_diag = g.dscale_col && dcol >= 0 && dcol < g.ncol && lane < g.nrow;
    double4_t acc[2][2];
    double dabs;
    if (st && threadIdx.x == 0) st[6] = ke - kb;
    if (pi < 0) {
        double old[2][2][4];
        gather_old(g, old);
        gather_acc_flat(p, recs, kb, ke, dcol, has_diag, acc, dabs, st);
        GST(4);
        gather_put(g, old, acc, dabs, has_diag, dcol);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        GST(5);
        return;
    }
    gather_acc_flat(p, recs, kb, ke, dcol, has_diag, acc, dabs, st);
    double* dst = partial + (size_t)pi * (TR * TR + 4 * TR);
    const int tid = threadIdx.x;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++) sc1_store(dst + ((a * 2 + b) * 4 + i) * NT + tid, acc[a][b][i]);
    sc1_store(dst + TR * TR + tid, dabs);
    __shared__ int last;
    const int q = ck_q[c];
    const int np = sp_n[q];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const int prev = __hip_atomic_fetch_add(split_cnt + q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = prev == np - 1;
        if (prev == np - 1) __hip_atomic_store(split_cnt + q, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!last) return;
    split_sum<SG>(partial, sp_p0[q], np, acc, dabs);
    gather_store(g, acc, dabs, has_diag, dcol);
}

// Quadrant gather for the level chain of deep trees.  Measured there
// (IPO_HIP_GATHER_STAMPS): a 64-slot flat round spends ~7.5 us staging its
// values -- the CU's outstanding misses, ~8 cache lines per slot from as
// many source columns -- not in the MFMA steps.  Here a unit's tile is
// gathered by up to four workgroups, one per 32 x 32 quadrant (the ones
// outside the tile or above the diagonal are not launched), each fetching
// only its 32 rows and 32 columns of every slot (lanes 0-31 the rows, 32-63
// the columns: one load per slot); wave w owns the quadrant's 16 x 16
// fragment (w & 1, w >> 1).  Every tile entry sees gather_acc's MFMA steps
// in its k order, and the diagonal's |terms| are summed in its four wave
// partials, so the factor is bitwise k_update's with one chunk per unit.
// ck_part holds -1 - quadrant (no split K: a quadrant loops over rounds).
__global__ void __launch_bounds__(NT)
k_update_quad(PlanView p, TailView tv, const SlotRec* __restrict__ recs, const int* __restrict__ ck_u,
              const int* __restrict__ ck_b, const int* __restrict__ ck_e, const int* __restrict__ ck_part, int c0,
              long long* __restrict__ stamps) {
    __shared__ double As[32][FK + 1];
    __shared__ double Bs[32][FK + 1];
    __shared__ SlotRec rl[FK];
    long long* st = stamps && blockIdx.x < 1024 ? stamps + blockIdx.x * 8 : nullptr;
    GST(0);
    const int c = c0 + blockIdx.x;
    const int u = ck_u[c], kb = ck_b[c], ke = ck_e[c], q = -1 - ck_part[c];
    const int qr = 32 * (q & 1), qc = 32 * (q >> 1);
    const GatherTile g = unit_tile(p, tv, u, -1);
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int fr = 16 * (wv & 1), fc = 16 * (wv >> 1);      // the wave's fragment inside the quadrant
    const int li = lane & 15, lk = lane >> 4;
    // the tile's old values of this lane's 4 fragment entries, before the gather
    double old[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int rr = qr + fr + lk + 4 * i, cc = qc + fc + li;
        const bool ok = rr < g.nrow && cc < g.ncol && g.row0 + rr >= g.col0 + cc;
        old[i] = ok ? g.out[rr + (size_t)cc * g.ld] : 0.0;
    }
    // diagonal quadrant of a tile with diagonal entries: wave 0's lanes < 32
    // keep the four wave partials of row qr + lane's |terms|
    const bool dq = g.dscale_col && qr == qc;
    const int drow = qr + (lane & 31), dcol = g.row0 + drow - g.col0;
    const bool has_diag = dq && wv == 0 && lane < 32 && dcol >= 0 && dcol < g.ncol && drow < g.nrow;
    double dp[4] = {0.0, 0.0, 0.0, 0.0};
    double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int half = lane >> 5, idx = lane & 31;
    const uint64_t bl = (1ull << ((half ? qc : qr) + idx)) - 1ull;
    const int bit = (half ? qc : qr) + idx;
    for (int k0 = kb; k0 < ke; k0 += FK) {
        const int nk = min(FK, ke - k0);
        if (tid < nk * 4)
            reinterpret_cast<uint64_t*>(rl)[tid] = reinterpret_cast<const uint64_t*>(recs + k0)[tid];
        __syncthreads();
        if (k0 == kb) GST(1);
        // wave w stages slots w, w + 4, ... (16 per 64-slot round, one load each)
        // every load issued before any is used (unconditional, clamped to the
        // slot's first entry; see slot_ld)
        double v[FK / 4], dv[FK / 4];
        bool on[FK / 4];
#pragma unroll
        for (int j = 0; j < FK / 4; j++) {
            const int k = min(wv + 4 * j, nk - 1);
            const SlotRec m = rl[k];
            const uint64_t mk = half ? m.cmask : m.rmask;
            on[j] = wv + 4 * j < nk && ((mk >> bit) & 1ull);
            v[j] = p.Lx[on[j] ? m.roff + (half ? m.cdelta : 0) + __popcll(mk & bl) : m.roff];
            dv[j] = p.dg[m.dk];
        }
#pragma unroll
        for (int j = 0; j < FK / 4; j++) v[j] = on[j] ? (half ? dv[j] * v[j] : v[j]) : 0.0;
#pragma unroll
        for (int j = 0; j < FK / 4; j++) {
            const int k = wv + 4 * j;
            if (k < nk) {
                if (half) Bs[idx][k] = v[j];
                else As[idx][k] = v[j];
            }
        }
        __syncthreads();
        if (k0 == kb) GST(2);
        for (int kk = 0; kk < nk; kk += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[fr + li][kk + lk], Bs[fc + li][kk + lk], acc, 0, 0, 0);
        if (has_diag) {
            // gather_acc's wave partials: wave w's slots k % 16 in [4w, 4w + 4)
            for (int sb = 0; sb < nk / KS; sb++)
#pragma unroll
                for (int w = 0; w < 4; w++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int k = sb * KS + w * 4 + j;
                        dp[w] += fabs(As[idx][k] * Bs[idx][k]);
                    }
        }
        __syncthreads();
        if (k0 == kb) GST(3);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int rr = qr + fr + lk + 4 * i, cc = qc + fc + li;
        if (rr < g.nrow && cc < g.ncol && g.row0 + rr >= g.col0 + cc) g.out[rr + (size_t)cc * g.ld] = old[i] - acc[i];
    }
    if (has_diag) g.dscale_col[dcol] += ((dp[0] + dp[1]) + dp[2]) + dp[3];
    if (st) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); GST(5); }
}

// ======================================================== dense tail
// S = Lx + off_tail, nt x nt column-major (ld = nt), columns tail_c0.. .
// (TailView is declared in kkt_device.h; the diagonal-block LDL' and the
// panel kernels: kkt_dense.hip)
//
// Trailing update S(bi, bj) -= L(bi, kb) * W(bj, kb)'  for bi >= bj > kb,
// with v_mfma_f64_16x16x4_f64: 4 waves, each a 32x32 quarter (2x2 MFMA tiles).
__global__ void __launch_bounds__(NT)
k_tail_syrk(PlanView p, TailView tv, int kb) {
    __shared__ double As[TR][PC + 1];    // L rows of block bi   [row][k]
    __shared__ double Bs[TR][PC + 1];    // W rows of block bj   [row][k]
    const int nb = tv.ntb - kb - 1;      // trailing blocks
    const int tile = blockIdx.x;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ti++;
    const int tj = tile - ti * (ti + 1) / 2;
    if (ti >= nb) return;
    const int bi = kb + 1 + ti, bj = kb + 1 + tj;
    const int k0 = kb * PC;
    const int nc = min(PC, tv.nt - k0);
    const int nt = tv.nt;
    const int tid = threadIdx.x;
    const double* Lcol = tv.S + (size_t)k0 * nt;      // column k0 of S
    // W rows are stored relative to the block column: W[(row - k0) + k * nt].
    // All 32 loads of a thread are issued before its first LDS store.
    {
        double va[TR * PC / NT], vb[TR * PC / NT];
#pragma unroll
        for (int u = 0; u < TR * PC / NT; u++) {
            const int idx = tid + u * NT, rr = idx % TR, k = idx / TR;
            const int ra = bi * TR + rr, rb = bj * TR + rr;
            const bool oka = k < nc && ra < nt, okb = k < nc && rb < nt;
            const double x = Lcol[oka ? ra + (size_t)k * nt : 0];
            const double y = tv.W[okb ? (rb - k0) + (size_t)k * nt : 0];
            va[u] = oka ? x : 0.0;
            vb[u] = okb ? y : 0.0;
        }
#pragma unroll
        for (int u = 0; u < TR * PC / NT; u++) {
            const int idx = tid + u * NT;
            As[idx % TR][idx / TR] = va[u];
            Bs[idx % TR][idx / TR] = vb[u];
        }
    }
    __syncthreads();
    const int wv = tid >> 6, lane = tid & 63;
    const int wr = (wv & 1) * 32, wc = (wv >> 1) * 32;
    double4_t acc[2][2];
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) acc[a][b] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int li = lane & 15, lk = lane >> 4;
    for (int kk = 0; kk < PC; kk += 4) {
        double av[2], bv[2];
        for (int a = 0; a < 2; a++) av[a] = As[wr + a * 16 + li][kk + lk];
        for (int b = 0; b < 2; b++) bv[b] = Bs[wc + b * 16 + li][kk + lk];
        for (int a = 0; a < 2; a++)
            for (int b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
    const bool diag_tile = bi == bj;
    double old[2][2][4];      // all loads before the first store (see gather_store)
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int rr = wr + a * 16 + (lane >> 4) + 4 * i;
                const int cc = wc + b * 16 + (lane & 15);
                const int rg = bi * TR + rr, cg = bj * TR + cc;
                const bool ok = rg < nt && cg < nt && !(diag_tile && cc > rr);
                old[a][b][i] = ok ? tv.S[rg + (size_t)cg * nt] : 0.0;
            }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int rr = wr + a * 16 + (lane >> 4) + 4 * i;
                const int cc = wc + b * 16 + (lane & 15);
                const int rg = bi * TR + rr, cg = bj * TR + cc;
                if (rg >= nt || cg >= nt || (diag_tile && cc > rr)) continue;
                tv.S[rg + (size_t)cg * nt] = old[a][b][i] - acc[a][b][i];
            }
    if (diag_tile && tid < TR) {           // |terms| of the diagonal for the zero-pivot test
        const int rg = bi * TR + tid;
        if (rg < nt) {
            double as = 0.0;
            for (int k = 0; k < nc; k++) as += fabs(As[tid][k] * Bs[tid][k]);
            p.dscale[tv.tc + rg] += as;
        }
    }
}

// -------------------------------------------------------- refinement glue
// The refinement pass's per-system launches, both active systems in one
// launch (blockIdx.y = the system's slot q; the refinement phase is
// host-bound, so a launch saved is time saved)
struct PermJobs {
    const double* fy[2];
    const double* fx[2];
    double* z[2];
    double* dy[2];
    double* dx[2];
    int mode[2];
};
// z[v] = rhs(perm[v]) with rhs = (fy | fx); the pass's first permutation also
// clears the consistency flags and the dropped-column eps of its sweep
// (zi[0..1], zd[0..1]; no fill launches)
__global__ void __launch_bounds__(NT)
k_perm_in2(int T, int m, const int* __restrict__ perm, PermJobs J, int* __restrict__ zi, double* __restrict__ zd) {
    const int v = blockIdx.x * NT + threadIdx.x, q = blockIdx.y;
    if (q == 0 && v < 2 && zi) { zi[v] = 0; zd[v] = 0.0; }
    if (v >= T) return;
    const int o = perm[v];
    J.z[q][v] = o < m ? J.fy[q][o] : J.fx[q][o - m];
}
// dy/dx (=|+=|-=) z[iperm[.]]
__global__ void __launch_bounds__(NT)
k_perm_out2(int T, int m, const int* __restrict__ iperm, PermJobs J) {
    const int o = blockIdx.x * NT + threadIdx.x, q = blockIdx.y;
    if (o >= T) return;
    const double v = J.z[q][iperm[o]];
    double* dst = o < m ? J.dy[q] + o : J.dx[q] + (o - m);
    const int mode = J.mode[q];
    if (mode == 0) *dst = v;
    else if (mode == 1) *dst = *dst + v;
    else *dst = *dst - v;
}

// dy/dx (=|+=|-=) z[iperm[.]]
__global__ void __launch_bounds__(NT)
k_perm_out(int T, int m, const int* __restrict__ iperm, const double* __restrict__ z, double* __restrict__ dy,
           double* __restrict__ dx, int mode) {
    const int o = blockIdx.x * NT + threadIdx.x;
    if (o >= T) return;
    const double v = z[iperm[o]];
    double* dst = o < m ? dy + o : dx + (o - m);
    if (mode == 0) *dst = v;
    else if (mode == 1) *dst = *dst + v;
    else *dst = *dst - v;
}

// KKT residual (ldlt.c:389-398):
//   ry_j = fy_j - ((A dx)_j - E_j dy_j)        row gather over CSR
//   rx_i = fx_i - ((A' dy)_i + D_i dx_i)       column gather over CSC
// plus max-abs partials of both (ldlt.c:401).
__device__ __forceinline__ void kkt_residual_body(
    int m, int n, const int* __restrict__ kAt, const int* __restrict__ iAt, const double* __restrict__ At,
    const int* __restrict__ kA, const int* __restrict__ iA, const double* __restrict__ A, const double* __restrict__ E,
    const double* __restrict__ D, const double* __restrict__ fy, const double* __restrict__ fx,
    const double* __restrict__ dy, const double* __restrict__ dx, double* __restrict__ ry, double* __restrict__ rx,
    double* __restrict__ part, int mrow, const double* __restrict__ axl, const int* __restrict__ kQ,
    const int* __restrict__ iQ, const double* __restrict__ Q, double qmax, int qthr,
    const double* __restrict__ qxl) {
    __shared__ double sh[kResThreads / 64];
    double mx = 0.0;
    for (int i = blockIdx.x * kResThreads + threadIdx.x; i < m + n; i += kRedBlocks * kResThreads) {
        if (i < m) {
            double s = 0.0;
            if (i >= mrow) s = axl[i - mrow];      // linking row: product summed over the shards
            else
                s = sparse_dot(kAt[i], kAt[i + 1], At, iAt, dx);
            // a Q block: fy - ((A dx - E dy) - max Q dy), ldlt.c:391-394
            // (Q symmetric: row i of Q dy summed over its column i in order;
            // a column of at least qthr entries by one wave beforehand, qxl)
            const double r = kQ ? fy[i] - ((s - E[i] * dy[i]) -
                                           qmax * (q_col_long(kQ, i, qthr) ? qxl[i]
                                                                           : sparse_dot(kQ[i], kQ[i + 1], Q, iQ, dy)))
                                : fy[i] - (s - E[i] * dy[i]);
            ry[i] = r;
            mx = fmax(mx, ref_abs(r));
        } else {
            const int j = i - m;
            double s = 0.0;
            s = sparse_dot(kA[j], kA[j + 1], A, iA, dy);
            const double r = fx[j] - (s + D[j] * dx[j]);
            rx[j] = r;
            mx = fmax(mx, ref_abs(r));
        }
    }
    mx = block_max_w<kResThreads / 64>(mx, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = mx;
}


struct ResJobs {
    const double* fy[2];
    const double* fx[2];
    const double* dy[2];
    const double* dx[2];
    double* ry[2];
    double* rx[2];
    const double* axl[2];
    const double* qxl[2];     // Q dy of the long columns of Q (launch_q_long), full length; null: none
};
// the active systems' residuals, one launch: system q = blockIdx.y writes
// the partials of slot q (part + q kRedBlocks)
__global__ void __launch_bounds__(kResThreads)
k_kkt_residual2(int m, int n, const int* __restrict__ kAt, const int* __restrict__ iAt, const double* __restrict__ At,
                const int* __restrict__ kA, const int* __restrict__ iA, const double* __restrict__ A,
                const double* __restrict__ E, const double* __restrict__ D, ResJobs J, double* __restrict__ part,
                int mrow, const int* __restrict__ kQ, const int* __restrict__ iQ, const double* __restrict__ Q,
                double qmax, int qthr) {
    const int q = blockIdx.y;
    kkt_residual_body(m, n, kAt, iAt, At, kA, iA, A, E, D, J.fy[q], J.fx[q], J.dy[q], J.dx[q], J.ry[q], J.rx[q],
                      part + (size_t)q * kRedBlocks, mrow, J.axl[q], kQ, iQ, Q, qmax, qthr, J.qxl[q]);
}

// -min|d| partials, so that the max-finisher yields -min|d| (negated on host)
__global__ void __launch_bounds__(NT)
k_min_abs_partial(const double* __restrict__ d, int T, double* __restrict__ part) {
    __shared__ double sh[4];
    double mn = HUGE_VAL;
    for (int i = blockIdx.x * NT + threadIdx.x; i < T; i += kRedBlocks * NT) mn = fmin(mn, ref_abs(d[i]));
    const double r = block_max(-mn, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// dst[2r] <- src[2r] (m values), dst[2r+1] <- src[2r+1] (n values), r < R
struct CopyOut {
    const double* src[4];
    double* dst[4];
    int m, n, R;
};
__global__ void __launch_bounds__(NT) k_copy_out(CopyOut c) {
    const int i = blockIdx.x * NT + threadIdx.x, per = c.m + c.n;
    if (i >= c.R * per) return;
    const int r = i / per, k = i - r * per;
    if (k < c.m) c.dst[2 * r][k] = c.src[2 * r][k];
    else c.dst[2 * r + 1][k - c.m] = c.src[2 * r + 1][k - c.m];
}
// n ints copied bit for bit into the doubles at out (one host read-back with them)
__global__ void k_pack_ints(const int* f, int n, double* out) {
    if (static_cast<int>(threadIdx.x) < n) reinterpret_cast<int*>(out)[threadIdx.x] = f[threadIdx.x];
}
__global__ void k_flag_to_scalar(const int* f, double* d) { d[0] = static_cast<double>(f[0]); }

}  // namespace

// ======================================================================
KktDevice::KktDevice(int m, int n, const int* kA, const int* iA, const double* A, hipStream_t stream, int nforced,
                     const QBlock* qb)
    : m_(m), n_(n), T_(m + n), nforced_(nforced), stream_(stream) {
    if (qb && !qb->kQ) qb = nullptr;
    if (qb && nforced > 0) throw std::invalid_argument("kkt: a Q block with forced rows is not supported");
    QPattern qpat;
    if (qb) { qpat.kQ = qb->kQ; qpat.iQ = qb->iQ; }
    const auto st0 = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {     // IPO_HIP_SETUP_TIMES: where the host setup goes, to stderr
        if (knobs_.setup_times)
            std::fprintf(stderr, "setup %-28s %9.1f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - st0).count());
    };
    std::vector<int> kat, iat;
    std::vector<double> at;
    csc_transpose(m, n, kA, iA, A, kat, iat, at);
    // the dense tail reaches down to the longest suffix at least 70 % full
    // (IPO_HIP_TAIL_DENSITY=1: only the reference's full dense window)
    const double tail_density = device_tail_density();
    mark("transpose");
    plan_ = build_kkt_plan(m, n, kA, iA, kat.data(), iat.data(), nforced, tail_density, qb ? &qpat : nullptr);
    mark("ordering + symbolic plan");
    h_.paths = kkt_paths(plan_, knobs_);
    int dev = 0, cus = 0;
    IPO_HIP_CHECK(hipGetDevice(&dev));
    IPO_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    upload_plan(kA, iA, A, kat, iat, at, qb);
    mark("upload_plan");
    build_panel_units();
    mark("build_panel_units");
    {
        const SolveChunks ch = build_solve_chunks();     // its per-supernode part, for the next two steps
        mark("build_solve_chunks");
        const SweepOrder so = build_sweep_order(ch);     // its per-level counts, for the sweeps' step lists
        mark("build_sweep_order");
        build_sync_free_plan(ch, so, cus);
        mark("build_sync_free_plan");
    }
    const VisitSlots vs = build_visit_slots(plan_, knobs_, h_.paths);
    mark("build_visit_slots");
    build_gather_chunks(vs);
    mark("build_gather_chunks");
    count_work();
    mark("count_work");
    build_slot_records(vs.kslot);
    mark("build_slot_records");
    setup_tail(cus);
    mark("setup_tail");
    alloc_numeric();
    mark("alloc_numeric");
}

// The constraint matrix in both orientations, the Q block and the plan's
// index arrays.  kat / iat / at and the plan outlive the constructor's first
// stream synchronisation; the Q diagonal is a local, synchronised here.
void KktDevice::upload_plan(const int* kA, const int* iA, const double* A, const std::vector<int>& kat,
                            const std::vector<int>& iat, const std::vector<double>& at, const QBlock* qb) {
    const int m = m_, n = n_;
    if (nforced_ > 0) dLinkAx_.alloc(2 * static_cast<size_t>(nforced_));
    const int nz = kA[n];
    hipStream_t s = stream_;
    dkA_.upload(kA, n + 1, s);
    diA_.upload(iA, nz, s);
    dA_.upload(A, nz, s);
    dkAt_.upload(kat, s);
    diAt_.upload(iat, s);
    dAt_.upload(at, s);
    {
        // where each entry of at came from (refresh_values): a local, synchronised here
        const std::vector<int> tmap = csr_value_map(m, n, kA, iA);
        dtmap_.upload(tmap, s);
        IPO_HIP_CHECK(hipStreamSynchronize(s));
    }

    dcol0_.upload(plan_.col0, s);
    drowptr_.upload(plan_.rowptr, s);
    drows_.upload(plan_.rows, s);
    dperm_.upload(plan_.perm, s);
    diperm_.upload(plan_.iperm, s);
    doff_.upload(plan_.off, s);
    damap_.upload(plan_.amap, s);
    if (qb) {
        qnz_ = qb->kQ[m];
        qmax_ = qb->qmax;
        dkQ_.upload(qb->kQ, m + 1, s);
        diQ_.upload(qb->iQ, qnz_ > 0 ? qnz_ : 1, s);
        dQ_.upload(qb->Q, qnz_ > 0 ? qnz_ : 1, s);
        dqmap_.upload(plan_.qmap, s);
        std::vector<double> qd(m > 0 ? m : 1, 0.0);
        for (int j = 0; j < m; j++)
            for (int k = qb->kQ[j]; k < qb->kQ[j + 1]; k++)
                if (qb->iQ[k] == j) qd[j] = qb->Q[k];
        dQdiag_.upload(qd, s);
        const std::vector<int> qdm = q_diag_map(m, qb->kQ, qb->iQ);
        dqdiagmap_.upload(qdm, s);
        // the long columns (kkt_device.h q_long_count), maybe none
        const std::vector<int> ql = q_long_columns(m, qb->kQ, knobs_.q_long);
        q_long_n_ = static_cast<int>(ql.size());
        if (q_long_n_ > 0) {
            dQLongCols_.upload(ql, s);
            dLongQ_.alloc(2 * static_cast<size_t>(m));
        }
        IPO_HIP_CHECK(hipStreamSynchronize(s));
    }
    ddslot_.upload(plan_.dslot, s);
    drelptr_.upload(plan_.relptr, s);
    dunit_sup_.upload(plan_.unit_sup, s);
    dunit_tile_.upload(plan_.unit_tile, s);
    dtask_ptr_.upload(plan_.task_ptr, s);
    dtask_pair_.upload(plan_.task_pair, s);
    dtask_i0_.upload(plan_.task_i0, s);
    dtask_i1_.upload(plan_.task_i1, s);
    dupd_src_.upload(plan_.upd_src, s);
    dupd_r0_.upload(plan_.upd_r0, s);
    dupd_r1_.upload(plan_.upd_r1, s);
    drel_.upload(plan_.rel, s);
    dlevel_sups_.upload(plan_.level_sups, s);
}

// New values on the same pattern (ipo_hip_ctx_update): dA in
// the constructor's CSC order and dQ in its kQ / iQ order, device arrays the
// caller has validated, either null for "unchanged".  Copies them over dA_ /
// dQ_ and regathers the CSR values and Q's diagonal through the maps built at
// construction; factor() scatters dA_ / dQ_ anew on every call.  Drops a
// pending pre-pass, resets nothing else.  Enqueued on the object's stream.
void KktDevice::refresh_values(const double* dA, const double* dQ) {
    hipStream_t s = stream_;
    const int nz = static_cast<int>(dtmap_.size());
    if (dA && nz > 0) {
        IPO_HIP_CHECK(hipMemcpyAsync(dA_.get(), dA, nz * sizeof(double), hipMemcpyDeviceToDevice, s));
        launch_gather_map(nz, dtmap_.get(), dA, dAt_.get(), s);
    }
    if (dQ) {
        if (qnz_ <= 0) throw std::invalid_argument("kkt: new Q values for a factor without a Q block");
        IPO_HIP_CHECK(hipMemcpyAsync(dQ_.get(), dQ, qnz_ * sizeof(double), hipMemcpyDeviceToDevice, s));
        launch_gather_map(m_, dqdiagmap_.get(), dQ, dQdiag_.get(), s);
    }
    drop_prepass();
}

// Fused panel units and small panels per level (kkt_schedule.h)
void KktDevice::build_panel_units() {
    hipStream_t s = stream_;
    PanelUnits pu = ipo::build_panel_units(plan_, knobs_, h_.paths);
    dfu_sup_.upload(pu.fu_sup, s);
    dfu_j_.upload(pu.fu_j, s);
    dsmall_sups_.upload(pu.small_sups, s);
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    h_.fu_ptr = std::move(pu.fu_ptr);
    h_.small_ptr = std::move(pu.small_ptr);
    h_.split_level = std::move(pu.split_level);
    h_.small1_cnt = std::move(pu.small1_cnt);
}

// Solve chunks of the chunked levels; returns what the sweep order and the
// sync-free plan read of them (the chunk lists themselves are dropped)
SolveChunks KktDevice::build_solve_chunks() {
    hipStream_t s = stream_;
    SolveChunks ch = ipo::build_solve_chunks(plan_);
    dchunk_sup_.upload(ch.chunk_sup, s);
    dchunk_r0_.upload(ch.chunk_r0, s);
    dsup_chunk0_.upload(ch.sup_chunk0, s);
    h_.partial_stride = ch.partial_stride;
    dPartial_.alloc(2 * h_.partial_stride);
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    ch.chunk_sup = {};
    ch.chunk_r0 = {};
    return ch;
}

// The sweep order of every level; returns its per-level leaf counts (the
// order itself is dropped once uploaded)
SweepOrder KktDevice::build_sweep_order(const SolveChunks& ch) {
    hipStream_t s = stream_;
    SweepOrder so = ipo::build_sweep_order(plan_, h_.paths, ch);
    dsweep_sups_.upload(so.sweep_sups, s);
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    so.sweep_sups = {};
    return so;
}

// Gather chunks (split K): groups = sparse levels (with their visits, vs),
// then the dense tail
void KktDevice::build_gather_chunks(const VisitSlots& vs) {
    hipStream_t s = stream_;
    GatherChunks g = ipo::build_gather_chunks(plan_, knobs_, h_.paths, vs);
    dck_u_.upload(g.ck_u, s);
    dck_b_.upload(g.ck_b, s);
    dck_e_.upload(g.ck_e, s);
    dck_part_.upload(g.ck_part, s);
    dsp_u_.upload(g.sp_u, s);
    dsp_p0_.upload(g.sp_p0, s);
    dsp_n_.upload(g.sp_n, s);
    dck_q_.upload(g.ck_q, s);
    dSplitCnt_.alloc(g.split_cnt);
    IPO_HIP_CHECK(hipMemsetAsync(dSplitCnt_.get(), 0, g.split_cnt * sizeof(int), s));
    dPartialTile_.alloc(g.partial_tiles * (kTileRows * kTileRows + 4 * kTileRows));
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    h_.ck_ptr = std::move(g.ck_ptr);
    h_.ck_kind = std::move(g.ck_kind);
    h_.ck_wide = std::move(g.ck_wide);
}

// Algorithmic work per phase occurrence (the sweeps' launches are counted
// where they are made, run_sweep_steps)
void KktDevice::count_work() {
    const WorkCounts w = ipo::count_work(plan_, knobs_, h_.sweep);
    std::copy(w.flops, w.flops + kNumPhases, work_flops);
    std::copy(w.bytes, w.bytes + kNumPhases, work_bytes);
}

// Per-task source descriptors and per-slot records of the gather; kslot_v:
// the sparse units' slots in visit order (build_visit_slots)
void KktDevice::build_slot_records(const std::vector<int>& kslot_v) {
    hipStream_t s = stream_;
    auto build = [&](const std::vector<TailTask>& ts, DevBuf<TaskSrc>& dst) {
        const std::vector<TaskSrc> v = build_task_src(plan_, ts);
        dst.upload(v, s);
        IPO_HIP_CHECK(hipStreamSynchronize(s));
    };
    build(plan_.utasks, dusrc_);
    if (plan_.nt > 0) build(plan_.tail_tasks, dtsrc_);
    auto expand = [&](const std::vector<int>& kslot, const std::vector<TailTask>& ts, DevBuf<SlotRec>& dst) {
        const std::vector<SlotRec> v = ipo::build_slot_records(plan_, kslot, ts);
        dst.upload(v, s);
        IPO_HIP_CHECK(hipStreamSynchronize(s));
    };
    expand(h_.paths.visits ? kslot_v : plan_.kslot, plan_.utasks, dslot_rec_);
    if (plan_.nt > 0) expand(plan_.tail_kslot, plan_.tail_tasks, dtail_slot_rec_);
    dutasks_.upload(reinterpret_cast<const uint64_t*>(plan_.utasks.data()), plan_.utasks.size() * 4, s);
}

// The dense tail: its task and slot lists, workspaces, the sweep chains'
// LDS attributes, the visit schedule and the persistent run's items and
// counters (cus: the device's CU count, one workgroup per CU per launch)
void KktDevice::setup_tail(int cus) {
    hipStream_t s = stream_;
    if (plan_.nt > 0) {
        dtail_task_ptr_.upload(plan_.tail_task_ptr, s);
        dtail_kslot_.upload(plan_.tail_kslot, s);
        dtail_kslot_ptr_.upload(plan_.tail_kslot_ptr, s);
        static_assert(sizeof(TailTask) == 32, "TailTask layout");
        dtail_tasks_.upload(reinterpret_cast<const uint64_t*>(plan_.tail_tasks.data()), plan_.tail_tasks.size() * 4, s);
        dW_.alloc(static_cast<size_t>(plan_.nt) * kPanelCols);   // W = L21 D of one block column (per-phase path)
        dDepSt_.alloc(tail_dep_state_doubles(plan_.ntb));
        dDepI_.alloc(8);
        // R <= 2 right-hand sides: z of every block, then k_tail_fwd_lead's helper partials
        dChainGran_.alloc(ChainGran::words(plan_.ntb));
        dlead_ticket_.alloc(1);
        IPO_HIP_CHECK(hipMemsetAsync(dlead_ticket_.get(), 0, sizeof(int), s));
        lead_ticket_next_ = 0;
        IPO_HIP_CHECK(hipMemsetAsync(dChainGran_.get(), 0, dChainGran_.bytes(), s));
    }
    raise_sweep_lds(false);
    if (plan_.nt > 0 && plan_.ntb <= kTailSchedMaxBlocks) {
        TailSchedule ts = build_tail_schedule(plan_, knobs_, h_.paths, cus);
        if (knobs_.visit_sched) {
            dvisit_list_.upload(ts.visit_list, s);
            IPO_HIP_CHECK(hipStreamSynchronize(s));   // ts is a local
            h_.visit_ptr = std::move(ts.visit_ptr);
        }
        if (h_.paths.tail_run) {
            static_assert(sizeof(SchedUint2) == sizeof(uint2), "SchedUint2 is uploaded as uint2");
            drun_items_.upload(reinterpret_cast<const uint2*>(ts.run_items.data()), ts.run_items.size(), s);
            h_.run_ptr = std::move(ts.run_ptr);
            drun_cnt_.alloc(RunCounters::words(plan_.ntb));
            // each step's tile windows handed to the next step's pre-update as
            // they complete (kkt_dense.hip RunPub; off: the pre-update waits
            // for the whole previous step and reads S)
            if (h_.paths.run_winpub) {
                drun_pub_.alloc(2 * static_cast<size_t>(plan_.ntb) * 4 * kTailPubWin);
                drun_wflag_.alloc(static_cast<size_t>(plan_.ntb) * plan_.ntb * 4);
                IPO_HIP_CHECK(hipMemsetAsync(drun_wflag_.get(), 0, drun_wflag_.bytes(), s));
                run_epoch_ = 0;
            }
            IPO_HIP_CHECK(hipStreamSynchronize(s));   // ts is a local
        }
    }
}

// The factor, its pivots and flags, the solve's vectors and scalars, events
void KktDevice::alloc_numeric() {
    hipStream_t s = stream_;
    dLx_.alloc(plan_.lx_size > 0 ? plan_.lx_size : 1);
    dDg_.alloc(T_ > 0 ? T_ : 1);
    dLive_.alloc(T_ > 0 ? T_ : 1);
    dDscale_.alloc(T_ > 0 ? T_ : 1);
    dFlags_.alloc(kFlagWords);
    IPO_HIP_CHECK(hipMemsetAsync(dFlags_.get(), 0, dFlags_.bytes(), s));
    dSign_.upload(plan_.dsign, s);
    dZ_.alloc(2 * (T_ > 0 ? T_ : 1));
    dDy_.alloc(2 * (m_ > 0 ? m_ : 1));
    dRy_.alloc(2 * (m_ > 0 ? m_ : 1));
    dDx_.alloc(2 * (n_ > 0 ? n_ : 1));
    dRx_.alloc(2 * (n_ > 0 ? n_ : 1));
    dIncons_.alloc(2);
    dPart_.alloc(8 * kRedBlocks);
    dScal_.alloc(kScCount);
    dFacScal_.alloc(kFsCount);
    static_assert(kFlagReadWords * sizeof(int) <= (kFsCount - kFsFlags) * sizeof(double), "the packed flag words");
    dPrePart_.alloc(8 * kRedBlocks);
    IPO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&hScal_), std::max(kScCount, kFsCount) * sizeof(double),
                                hipHostMallocDefault));
    IPO_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&hDepDone_), sizeof(int), hipHostMallocDefault));
    IPO_HIP_CHECK(hipEventCreate(&ev0_));
    IPO_HIP_CHECK(hipEventCreate(&ev1_));
    IPO_HIP_CHECK(hipEventCreate(&ev2_));
    IPO_HIP_CHECK(hipEventCreate(&ev3_));
    IPO_HIP_CHECK(hipEventCreateWithFlags(&ev_pre_fork_, hipEventDisableTiming));
    IPO_HIP_CHECK(hipEventCreateWithFlags(&ev_pre_done_, hipEventDisableTiming));
    IPO_HIP_CHECK(hipEventCreateWithFlags(&ev_run_reset_, hipEventDisableTiming));
    IPO_HIP_CHECK(hipStreamSynchronize(s));
}

// Sync-free top levels of the sweeps (kkt_schedule.h): the forward update
// lists (yrow_ptr as the plan's, yrow_idx with the moved slices), the padded
// slices, the items and their counters; then, every fact they depend on being
// known, the sweeps' step lists (h_.sweep).  cus: the device's CU count, the
// sweeps' grid.
void KktDevice::build_sync_free_plan(const SolveChunks& ch, const SweepOrder& so, int cus) {
    hipStream_t s = stream_;
    dyrow_ptr_.upload(plan_.yrow_ptr, s);
    const SyncFreePlan sf = ipo::build_sync_free_plan(plan_, knobs_, h_.paths, ch);
    const int ns = plan_.nsup;
    h_.sf_level = sf.sf_level;
    dyrow_idx_.upload(sf.yrow_idx, s);
    dybase_.upload(sf.ybase, s);
    if (sf.late_lists) {
        dylate_ptr_.upload(sf.ylate_ptr, s);
        dylate_idx_.upload(sf.ylate_idx.empty() ? std::vector<int>{0} : sf.ylate_idx, s);
        dpre_col_.upload(sf.pre_col.empty() ? std::vector<int>{0} : sf.pre_col, s);
        dpre_ptr_.upload(sf.pre_ptr, s);
        dpre_idx_.upload(sf.pre_idx.empty() ? std::vector<int>{0} : sf.pre_idx, s);
        IPO_HIP_CHECK(hipStreamSynchronize(s));
    }
    h_.ybuf_stride = sf.ybuf_stride;
    dYbuf_.alloc(2 * h_.ybuf_stride);
    h_.sweep = build_sweep_steps(plan_, knobs_, h_.paths, ch, so, sf, h_.paths.tail_blocked);
    if (sf.range(plan_)) {
        static_assert(sizeof(SchedInt2) == sizeof(int2), "SchedInt2 is uploaded as int2");
        dsf_items_f_.upload(reinterpret_cast<const int2*>(sf.items_f.data()), sf.items_f.size(), s);
#ifdef IPO_SF_STAMPS
        h_sf_items_f_ = sf.items_f;
#endif
        dsf_items_b_.upload(reinterpret_cast<const int2*>(sf.items_b.data()), sf.items_b.size(), s);
        dsf_need_.upload(sf.need, s);
        dsf_par_.upload(sf.par, s);
        dsf_zbase_.upload(sf.zbase, s);
        dsf_zpi_.upload(sf.zpi, s);
        h_.zpad_stride = sf.zpad_stride;
        dZpad_.alloc(2 * h_.zpad_stride);
        for (DevBuf<int>* b : {&dsf_fcnt_, &dsf_fflag_, &dsf_bcnt_, &dsf_bflag_}) {
            b->alloc(ns);
            IPO_HIP_CHECK(hipMemsetAsync(b->get(), 0, ns * sizeof(int), s));
        }
        dsf_ticket_.alloc(2);
        IPO_HIP_CHECK(hipMemsetAsync(dsf_ticket_.get(), 0, 2 * sizeof(int), s));
        sf_ticket_next_[0] = sf_ticket_next_[1] = 0;
        sf_grid_ = cus;
    }
    raise_sweep_lds(true);
    IPO_HIP_CHECK(hipStreamSynchronize(s));   // sf is a local
}

KktDevice::~KktDevice() {
    dump_sf_stamps();
    if (knobs_.debug_redo)
        std::fprintf(stderr, "kkt: %ld factorisations, %ld redone; bails (unused) %ld, k_panel_w sparse %ld, tail %ld, "
                             "k_panel_s %ld; tail block columns repaired %ld in %ld rounds\n", tm_.factors,
                     tm_.panel_redos, tm_.redo_where[0], tm_.redo_where[1], tm_.redo_where[2], tm_.redo_where[3],
                     tm_.tail_repairs, tm_.tail_dep_rounds);
    if (knobs_.debug_redo) {
        std::fprintf(stderr, "kkt: forward pre-passes used %ld, discarded %ld\n", pre_used_, pre_discarded_);
        std::fprintf(stderr, "kkt: trailing leads used %ld, discarded %ld\n", lead_used_, lead_discarded_);
    }
    if (hScal_) (void)hipHostFree(hScal_);
    if (hDepDone_) (void)hipHostFree(hDepDone_);
    if (ev0_) (void)hipEventDestroy(ev0_);
    if (ev1_) (void)hipEventDestroy(ev1_);
    if (ev2_) (void)hipEventDestroy(ev2_);
    if (ev3_) (void)hipEventDestroy(ev3_);
    if (ev_pre_fork_) (void)hipEventDestroy(ev_pre_fork_);
    if (ev_pre_done_) (void)hipEventDestroy(ev_pre_done_);
    if (ev_run_reset_) (void)hipEventDestroy(ev_run_reset_);
    for (hipEvent_t e : kev_) (void)hipEventDestroy(e);
}

PlanView KktDevice::plan_view() const {
    PlanView v;
    v.col0 = dcol0_.get(); v.rowptr = drowptr_.get(); v.rows = drows_.get(); v.off = doff_.get();
    v.unit_sup = dunit_sup_.get(); v.unit_tile = dunit_tile_.get();
    v.task_ptr = dtask_ptr_.get(); v.task_pair = dtask_pair_.get();
    v.task_i0 = dtask_i0_.get(); v.task_i1 = dtask_i1_.get();
    v.upd_src = dupd_src_.get(); v.upd_r0 = dupd_r0_.get(); v.upd_r1 = dupd_r1_.get();
    v.relptr = drelptr_.get(); v.rel = drel_.get();
    v.Lx = dLx_.get(); v.dg = dDg_.get(); v.live = dLive_.get();
    v.flags = dFlags_.get();
    v.sign = dSign_.get();
    v.xcd = knobs_.update_xcd;     // gather launches of at least this many chunks walk them XCD by XCD (0: off)
    v.dscale = dDscale_.get();
    v.tau = pivot_tol_;
    v.incons = dIncons_.get();
    v.ybase = dybase_.get();
    return v;
}

TailView KktDevice::tail_view() const {
    TailView t;
    t.S = dLx_.get() + plan_.off_tail;
    t.nt = plan_.nt;
    t.ntb = plan_.ntb;
    t.tc = plan_.tail_c0;
    t.task_ptr = dtail_task_ptr_.get();
    t.tasks = reinterpret_cast<const TailTask*>(dtail_tasks_.get());
    t.W = dW_.get();
    t.vk = knobs_.visit_blocks;
    if (!h_.visit_ptr.empty()) {
        t.vlist = dvisit_list_.get();
        t.vptr = h_.visit_ptr.data();
    }
    // dependent pivots in the look-ahead panel: its failed checks fall back on
    // the host repair, which the sharded solve does not use
    t.dep = tail_repair() ? knobs_.tail_spec : 0;
    // in the sparse panels a failed check falls back on redoing the factor
    // from the assembly, on every shard alike (the bail flags are reduced)
    t.sdep = knobs_.sparse_dep;
    return t;
}

// Developer diagnostics (IPO_HIP_DUMP_DIR=dir): every factorisation's input
// (E, D, eps_diag) and outcome (live marks, D, |terms| sums, ndep) to
// dir/fNNNN.bin, for tools/dep_compare.py, which refactors the same input
// with the oracle and compares the dependent-pivot classification.
// Layout: int32 m, n, T, ndep; f64 eps_in, eps_out; f64 E[m], D[n];
// int32 perm[T]; int32 live[T]; f64 dg[T]; f64 dscale[T] (new order).
void KktDevice::dump_factor(const double* dE, const double* dD, double eps_in) {
    if (knobs_.dump_dir.empty()) return;
    std::vector<double> E(m_), D(n_), dg(T_), dsc(T_);
    std::vector<int> live(T_);
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
    if (m_) IPO_HIP_CHECK(hipMemcpy(E.data(), dE, m_ * sizeof(double), hipMemcpyDeviceToHost));
    if (n_) IPO_HIP_CHECK(hipMemcpy(D.data(), dD, n_ * sizeof(double), hipMemcpyDeviceToHost));
    dLive_.download(live.data(), T_, stream_);
    dDg_.download(dg.data(), T_, stream_);
    dDscale_.download(dsc.data(), T_, stream_);
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
    char path[4096];
    std::snprintf(path, sizeof path, "%s/f%04d.bin", knobs_.dump_dir.c_str(), dump_count_++);
    FILE* f = std::fopen(path, "wb");
    if (!f) return;
    const int hdr[4] = {m_, n_, T_, ndep_};
    const double eps[2] = {eps_in, epsdiag_};
    std::fwrite(hdr, sizeof(int), 4, f);
    std::fwrite(eps, sizeof(double), 2, f);
    std::fwrite(E.data(), sizeof(double), m_, f);
    std::fwrite(D.data(), sizeof(double), n_, f);
    std::fwrite(plan_.perm.data(), sizeof(int), T_, f);
    std::fwrite(live.data(), sizeof(int), T_, f);
    std::fwrite(dg.data(), sizeof(double), T_, f);
    std::fwrite(dsc.data(), sizeof(double), T_, f);
    std::fclose(f);
}

void KktDevice::factor(const double* dE, const double* dD, const PrePass* pre) {
    const double eps_in = epsdiag_;
    drop_prepass();               // one whose factor no solve followed
    try {
        factor_core(dE, dD, pre);
    } catch (...) {
        // an enqueued pre-pass is not used, and what follows on the object's
        // stream comes after it (its done event is recorded already)
        if (pre_state_ != kPreNone) (void)hipStreamWaitEvent(stream_, ev_pre_done_, 0);
        drop_prepass();
        throw;
    }
    dump_factor(dE, dD, eps_in);
}

void KktDevice::factor_core(const double* dE, const double* dD, const PrePass* pre) {
    // fast path: fused diagonal-block + panel kernels; a pivot that fails
    // the zero test makes them stop unwritten.  A bail in the dense tail
    // only: the look-ahead resumes from the bailed block column (repair);
    // in the sparse levels: the factorisation is redone with the per-phase
    // kernels there, which own the dependent-pivot rule, and the tail again
    // by the look-ahead (its own bails repaired the same way) -- a per-phase
    // tail costs a single-workgroup partial substitution per block column
    const bool repair = tail_repair();
    const bool ok = factor_pass(dE, dD, use_panel_, use_panel_, pre);
    if (!ok) {
        tm_.panel_redos++;
        for (int b = 0; b < 4; b++) tm_.redo_where[b] += (verdict_.bail >> b) & 1;
        if (repair && verdict_.tail_only()) repair_tail();
        else if (!factor_pass(dE, dD, false, repair) && repair && verdict_.tail_only()) repair_tail();
    }
    tm_.factors++;
    // one occurrence per factorisation, whatever redos and repairs it took
    // (their launches and time stay in the phases: the work is priced once)
    if (timing_)
        for (int ph : {kPhGather, kPhDiag, kPhTrsm, kPhSyrk, kPhTail}) tm_.phase_count[ph]++;
    ndep_ = verdict_.ndep_all;
    // the pre-pass stands if the first pass did (no redo, no repair) and no
    // pivot was dropped: it ran with eps = 0, which only a factor without
    // dropped columns never reads (rawsolve, ldlt.c:446)
    if (pre_state_ == kPreEnqueued) {
        if (ok && ndep_ == 0) pre_state_ = kPreValid;
        else drop_prepass();
    }
    if (verdict_.min_d < 1.0e-14) epsdiag_ *= 10;
    // developer diagnostics (IPO_HIP_EPSDIAG_MAX, tools/status_loss_probe.py):
    // a cap on the growth above, to measure what a stalled solve owes to it
    if (knobs_.epsdiag_max > 0.0 && epsdiag_ > knobs_.epsdiag_max) epsdiag_ = knobs_.epsdiag_max;
}

// One numeric factorisation, the sparse levels by the fused kernels (fused)
// or the per-phase ones, the dense tail by the look-ahead (tail_fused) or
// the per-phase kernels; returns false when fused kernels bailed out
// (verdict_.bail says where; nothing of a bailed part may then be used).
bool KktDevice::factor_pass(const double* dE, const double* dD, bool fused, bool tail_fused, const PrePass* pre) {
    hipStream_t s = stream_;
    if (timing_) IPO_HIP_CHECK(hipEventRecord(ev0_, s));
    const PlanView pv = plan_view();
    const int nz = static_cast<int>(plan_.amap.size());
    if (plan_.nt > 0 && !xch_) {
        // the sparse panels, then the tail's lower block triangle only (the
        // sharded solve sums the whole tail across shards: cleared whole)
        if (plan_.off_tail > 0) IPO_HIP_CHECK(hipMemsetAsync(dLx_.get(), 0, plan_.off_tail * sizeof(double), s));
        hipLaunchKernelGGL(k_zero_tail_lower, dim3(plan_.nt), dim3(NT), 0, s, dLx_.get() + plan_.off_tail, plan_.nt);
    } else {
        IPO_HIP_CHECK(hipMemsetAsync(dLx_.get(), 0, dLx_.bytes(), s));
    }
    if (nz > 0) hipLaunchKernelGGL(k_assemble_A, dim3(ceil_div(nz, NT)), dim3(NT), 0, s, nz, dA_.get(), damap_.get(), dLx_.get());
    if (qnz_ > 0)
        hipLaunchKernelGGL(k_assemble_Q, dim3(ceil_div(qnz_, NT)), dim3(NT), 0, s, qnz_, dQ_.get(), dqmap_.get(),
                           static_cast<double>(qmax_), dLx_.get());
    hipLaunchKernelGGL(k_assemble_diag, dim3(ceil_div(T_, NT)), dim3(NT), 0, s, T_, m_, dperm_.get(), dE, dD, epsdiag_,
                       ddslot_.get(), dLx_.get(), dLive_.get(), dDscale_.get(), shard_minor() ? plan_.tail_c0 : T_,
                       dFlags_.get(), dkQ_.get() ? dQdiag_.get() : static_cast<const double*>(nullptr),
                       static_cast<double>(qmax_));
    const TailView tv = tail_view();
    if (!prepass_eligible(pre, fused, tail_fused)) pre = nullptr;
    enqueue_levels(pv, tv, fused, s, pre);
    if (plan_.nt > 0) {
        // shards: S = sum of every shard's assembled + gathered tail (exchange.h)
        xsum(tv.S, static_cast<size_t>(plan_.nt) * plan_.nt, RedOp::Sum);
        xsum(dDscale_.get() + plan_.tail_c0, plan_.nt, RedOp::Sum);
        if (tail_fused && h_.paths.tail_run) {     // one persistent launch (kkt_dense.hip, k_tail_run)
            launch_tail_from(0, true);
        } else if (tail_fused) {     // look-ahead steps (kkt_dense.hip, k_tail_pr)
            // one event pair around the steps (a pair per launch added its
            // own ~2.5 us to every launch's time: the phase's average launch
            // would not be the kernel's)
            ph_begin(s);
            for (int t = 0; t < plan_.ntb; t++) launch_tail_step(pv, tv, t, s);
            ph_end(kPhTail, plan_.ntb, s);
        } else
        for (int kb = 0; kb < plan_.ntb; kb++) {
            const int k0 = kb * kPanelCols, nc = std::min(kPanelCols, plan_.nt - k0);
            const int below = plan_.nt - k0 - nc;
            ph_begin(s);
            {
                launch_diag(pv, nullptr, 0, 1, tv, kb, s);
                ph_end(kPhDiag, 1, s);
                if (below > 0) {
                    ph_begin(s);
                    launch_trsm(pv, 0, -1, tv, kb, s);
                    ph_end(kPhTrsm, 1, s);
                }
            }
            if (below > 0) {
                const int nb = plan_.ntb - kb - 1;
                ph_begin(s);
                hipLaunchKernelGGL(k_tail_syrk, dim3(nb * (nb + 1) / 2), dim3(NT), 0, s, pv, tv, kb);
                ph_end(kPhSyrk, 1, s);
            }
        }
    }
    // The pre-pass joins the object's stream here, behind the tail's factor
    // (ten times its length on dfl001): finish_pass's synchronisation then
    // covers it, so whatever follows a factorisation on either stream -- a
    // redo, a repair, a solve that does not use it, the next factorisation,
    // an exception's unwinding -- finds its buffers at rest.
    if (pre) IPO_HIP_CHECK(hipStreamWaitEvent(s, ev_pre_done_, 0));
    return finish_pass(fused || tail_fused);
}

// Whether this pass of the factorisation takes the caller's pre-pass request:
// the first pass only (factor_core passes the request to no other), fused
// panels and the persistent tail, a forward list with a TailGather / TailLead
// pair, one GPU, no timing mode (its phase events would time two streams).
bool KktDevice::prepass_eligible(const PrePass* pre, bool fused, bool tail_fused) const {
    return knobs_.prepass && pre && (pre->R == 1 || pre->R == 2) && pre->stream && pre->stream != stream_ &&
           pre->ready && fused && tail_fused && h_.paths.tail_run && h_.sweep.split > 0 && !xch_ && !timing_;
}

// The head of a solve's first refinement pass for R right-hand sides, on s:
// maxbc_r = MAX(maxv(fx_r), maxv(fy_r)) + 1 (ldlt.c:367) into dScal_'s kScMaxbc,
// read back with the pass's residuals (no copy or wait of its own), and the
// right-hand sides permuted into dZ_ (k_perm_in2, which also clears the
// sweep's eps slots and consistency flags).  part: the reduction's partials.
void KktDevice::enqueue_pass_head(int R, double* const* dfy, double* const* dfx, double* part, hipStream_t s) {
    RedJobs j{};
    j.nj = 2 * R;
    PermJobs J{};
    for (int r = 0; r < R; r++) {
        j.a[2 * r] = dfx[r]; j.b[2 * r] = nullptr; j.len[2 * r] = n_; j.op[2 * r] = 1;
        j.a[2 * r + 1] = dfy[r]; j.b[2 * r + 1] = nullptr; j.len[2 * r + 1] = m_; j.op[2 * r + 1] = 1;
        J.fy[r] = dfy[r];
        J.fx[r] = dfx[r];
        J.z[r] = dZ_.get() + static_cast<size_t>(r) * T_;
    }
    launch_reduce(j, part, dScal_.get() + kScMaxbc, s);
    xsum(dScal_.get() + kScMaxbc, 2 * R, RedOp::Max);
    hipLaunchKernelGGL(k_perm_in2, dim3(ceil_div(T_, NT), R), dim3(NT), 0, s, T_, m_, dperm_.get(), J, dIncons_.get(),
                       sweep_eps());
}

// The forward pre-pass (kkt_device.h PrePass), forked off the object's stream
// where it stands: behind the last sparse panel.  What it touches, against
// what the object's stream runs meanwhile (the tail's gather, k_tail_run,
// finish_pass after the join): DESIGN.md 6.5.
void KktDevice::enqueue_prepass(const PrePass& pre) {
    hipStream_t q = pre.stream;
    IPO_HIP_CHECK(hipEventRecord(ev_pre_fork_, stream_));
    IPO_HIP_CHECK(hipStreamWaitEvent(q, ev_pre_fork_, 0));
    IPO_HIP_CHECK(hipStreamWaitEvent(q, pre.ready, 0));
    enqueue_pass_head(pre.R, pre.dfy, pre.dfx, dPrePart_.get(), q);
    run_prepass_steps(pre.R, q);
    IPO_HIP_CHECK(hipEventRecord(ev_pre_done_, q));
    pre_req_ = pre;
    pre_state_ = kPreEnqueued;
    // the lead too, behind or beside the run: launch_tail_from(0, true)
    // enqueues it (mode 2 records ev_pre_done_ again, after it)
    pre_lead_ = false;
    lead_pending_ = h_.sweep.lead_end > 0 ? knobs_.lead_trail_mode(plan_.ntb) : 0;
}

// The sparse levels (gather, then panels, level by level) and the dense
// tail's gather of one factorisation, enqueued on s.
void KktDevice::enqueue_levels(const PlanView& pv, const TailView& tv, bool fused, hipStream_t s, const PrePass* pre) {
    for (int l = 0; l < plan_.nlevels; l++) {
        const int u0 = plan_.unit_level_ptr[l], u1 = plan_.unit_level_ptr[l + 1];
        if (u1 <= u0) continue;
        if (l > 0) {
            ph_begin(s);
            const int nl = launch_gather(pv, tv, -1, l, s);
            ph_end(kPhGather, nl, s);
        }
        const int q0 = plan_.level_ptr[l], q1 = plan_.level_ptr[l + 1];
        ph_begin(s);
        if (fused && h_.split_level[l]) {
            launch_diag(pv, dlevel_sups_.get(), q0, q1 - q0, tv, 0, s);
            launch_trsm(pv, u0, u1 - u0, tv, 0, s);
            ph_end(kPhDiag, 2, s);
        } else if (fused) {
            const int nsm = h_.small_ptr[l + 1] - h_.small_ptr[l], nfu = h_.fu_ptr[l + 1] - h_.fu_ptr[l];
            const int n1 = h_.small1_cnt[l];
            if (knobs_.merge_levels && nfu > 0 && nsm > n1) {
                launch_panel_small(pv, dsmall_sups_.get(), h_.small_ptr[l], n1, tv.sdep, s, n1);
                launch_panel_ws(pv, dfu_sup_.get(), dfu_j_.get(), h_.fu_ptr[l], nfu, tv, dsmall_sups_.get(),
                                h_.small_ptr[l] + n1, nsm - n1, tv.sdep, s);
                ph_end(kPhDiag, 1 + (n1 > 0), s);
            } else {
                launch_panel_small(pv, dsmall_sups_.get(), h_.small_ptr[l], nsm, tv.sdep, s, n1);
                launch_panel(pv, dfu_sup_.get(), dfu_j_.get(), h_.fu_ptr[l], nfu, tv, -1, s);
                ph_end(kPhDiag, (nsm > 0) + (nfu > 0), s);
            }
        } else {
            launch_diag(pv, dlevel_sups_.get(), q0, q1 - q0, tv, 0, s);
            ph_end(kPhDiag, 1, s);
            ph_begin(s);
            launch_trsm(pv, u0, u1 - u0, tv, 0, s);
            ph_end(kPhTrsm, 1, s);
        }
    }
    if (pre) enqueue_prepass(*pre);       // the sparse panels are final from here on
    if (plan_.nt > 0) {
        ph_begin(s);
        const int nl = launch_gather(pv, tv, 0, plan_.nlevels, s);
        ph_end(kPhGather, nl, s);
    }
}

// min |d| over the factor (ldlt.c:293-306), the dependent-pivot count and
// the fused kernels' bail-out flags, to the host
bool KktDevice::finish_pass(bool fused) {
    hipStream_t s = stream_;
    IPO_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_min_abs_partial, dim3(kRedBlocks), dim3(NT), 0, s, dDg_.get(), T_, dPart_.get());
    if (xch_) {   // every shard must take the same eps_diag / dependent-pivot / redo decisions
        static_assert(kFsNegMinD == 0 && kFsNdepMax == 1 && kFsBailMax == 2, "one allreduce over the three");
        hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, dPart_.get(), 1, 1u,
                           dFacScal_.get() + kFsNegMinD);
        hipLaunchKernelGGL(k_flag_to_scalar, dim3(1), dim3(1), 0, s, dFlags_.get() + kFlagNdep,
                           dFacScal_.get() + kFsNdepMax);
        hipLaunchKernelGGL(k_flag_to_scalar, dim3(1), dim3(1), 0, s, dFlags_.get() + kFlagBail,
                           dFacScal_.get() + kFsBailMax);
        xsum(dFacScal_.get(), kFsFlags, RedOp::Max);
        hipLaunchKernelGGL(k_pack_ints, dim3(1), dim3(kFlagReadWords), 0, s, dFlags_.get(), kFlagReadWords,
                           dFacScal_.get() + kFsFlags);
    } else {
        // min|d| and the three flags in one read-back, one launch
        hipLaunchKernelGGL(k_finish_reduce_pack, dim3(1), dim3(kRedThreads), 0, s, dPart_.get(), 1, 1u,
                           dFacScal_.get() + kFsNegMinD, static_cast<const int*>(dFlags_.get()), kFlagReadWords,
                           dFacScal_.get() + kFsFlags);
    }
    IPO_HIP_CHECK(hipMemcpyAsync(hScal_, dFacScal_.get(), kFsCount * sizeof(double), hipMemcpyDeviceToHost, s));
    if (timing_) IPO_HIP_CHECK(hipEventRecord(ev1_, s));
    IPO_HIP_CHECK(hipStreamSynchronize(s));
    if (gst_n_ > 0) {      // developer stamps of one gather launch (IPO_HIP_GATHER_STAMPS)
        std::vector<long long> st(1024 * 8);
        IPO_HIP_CHECK(hipMemcpy(st.data(), dGStamp_.get(), st.size() * sizeof(long long), hipMemcpyDeviceToHost));
        long long t0 = st[0];
        for (int b = 0; b < std::min(gst_n_, 1024); b++) t0 = std::min(t0, st[b * 8]);
        std::fprintf(stderr, "gather stamps group %d, %d workgroups (us from first start: start rec val mfma acc put slots)\n",
                     gst_group_, gst_n_);
        for (int b = 0; b < std::min(gst_n_, 1024); b++) {
            const long long* q = st.data() + b * 8;
            std::fprintf(stderr, "  wg %4d: %6.2f %6.2f %6.2f %6.2f %6.2f %6.2f  %lld\n", b, (q[0] - t0) / 100.0,
                         (q[1] - t0) / 100.0, (q[2] - t0) / 100.0, (q[3] - t0) / 100.0, (q[4] - t0) / 100.0,
                         (q[5] - t0) / 100.0, q[6]);
        }
        gst_n_ = 0;
        gst_group_ = -1;
    }
    {
        int f[kFlagReadWords];
        std::memcpy(f, hScal_ + kFsFlags, sizeof(f));
        FactorVerdict& v = verdict_;
        v.min_d = -hScal_[kFsNegMinD];
        v.ndep = f[kFlagNdep];
        v.bail = f[kFlagBail];
        v.tail_block = f[kFlagTailBlock];
        v.ndep_all = xch_ ? static_cast<int>(hScal_[kFsNdepMax]) : v.ndep;
        v.bail_all = xch_ ? static_cast<int>(hScal_[kFsBailMax]) : v.bail;
    }
    if (timing_) {
        float ms = 0;
        IPO_HIP_CHECK(hipEventElapsedTime(&ms, ev0_, ev1_));
        tm_.factor_ms += ms;
        ph_collect();
    }
    return !(fused && verdict_.any_bail());
}

// The dense tail's look-ahead steps [t0, ntb) as one persistent launch
// (k_tail_run).  reset: the factorisation's first run (every counter
// zeroed); a run resumed by repair_tail keeps pdone / vseq, which hold
// exactly the items of launches <= tb (later items were skipped uncounted).
void KktDevice::launch_tail_from(int t0, bool reset) {
    hipStream_t s = stream_;
    const PlanView pv = plan_view();
    const RunCounters cnt = run_counters();
    // every counter (the ticket comes first), or the ticket alone
    const size_t ncnt = reset ? RunCounters::words(plan_.ntb) : 1;
    IPO_HIP_CHECK(hipMemsetAsync(cnt.ticket, 0, ncnt * sizeof(int), s));
    TailRun rc;
    rc.items = drun_items_.get() + h_.run_ptr[t0];
    rc.n = h_.run_ptr[plan_.ntb] - h_.run_ptr[t0];
    rc.t0 = t0;
    rc.ticket = cnt.ticket;
    rc.pdone = cnt.pdone;
    rc.vseq = cnt.vseq;
    rc.cdone = cnt.cdone;
    if (h_.paths.run_winpub) {
        if (run_epoch_ == INT_MAX) {      // (never within a process's life: one epoch per factorisation)
            IPO_HIP_CHECK(hipMemsetAsync(drun_wflag_.get(), 0, drun_wflag_.bytes(), s));
            run_epoch_ = 0;
        }
        rc.pub = drun_pub_.get();
        rc.wflag = drun_wflag_.get();
        rc.pread = cnt.pread;
        // a resumed run: steps >= t0 count their readers afresh
        if (!reset) IPO_HIP_CHECK(hipMemsetAsync(rc.pread + t0, 0, (plan_.ntb - t0) * sizeof(int), s));
        rc.epoch = ++run_epoch_;
    }
    // the trailing lead beside the run (IPO_HIP_LEAD_TRAIL=2) starts once
    // the counters above are reset
    if (lead_pending_ == 2) IPO_HIP_CHECK(hipEventRecord(ev_run_reset_, s));
    ph_begin(s);
    launch_tail_run(pv, tail_view(), rc, s);
    ph_end(kPhTail, rc.n > 0, s);
    // The pre-pass's forward lead in its trailing form, enqueued after the
    // run (a failed run launch has thrown above and leaves no poller behind):
    // behind it on this stream (1), or beside it on the pre-pass's stream
    // (2), where ev_pre_done_ is recorded after it, so the wait before
    // finish_pass still leaves both streams at rest.
    if (lead_pending_) {
        hipStream_t q = lead_pending_ == 2 ? pre_req_.stream : s;
        if (lead_pending_ == 2) IPO_HIP_CHECK(hipStreamWaitEvent(q, ev_run_reset_, 0));
        else IPO_HIP_CHECK(hipStreamWaitEvent(q, ev_pre_done_, 0));     // the pre-pass's gather of the tail's z
        launch_lead_trail(pre_req_.R, q, lead_pending_ == 2);
        if (lead_pending_ == 2) IPO_HIP_CHECK(hipEventRecord(ev_pre_done_, q));
        pre_lead_ = true;
        lead_pending_ = 0;
    }
}

// The look-ahead dense tail bailed at block column tb (a pivot failed the
// zero test; launches after it did nothing): the sparse factor and block
// columns < tb stand, column tb holds the updates of blocks <= tb - 2 (its
// panel stores S only once it holds) and every column right of it what its
// visits up to launch tb gave it.  Apply block tb - 1 to column tb, factor
// column tb with the dependent-pivot rounds (k_tail_dep), and resume
// the look-ahead at tb + 1 with the same visit schedule: the fast path's
// operations with block column tb's panel replaced by k_diag + k_trsm.
// Repeats while a later column bails.
void KktDevice::repair_tail() {
    hipStream_t s = stream_;
    const PlanView pv = plan_view();
    for (;;) {
        const int tb = verdict_.tail_col();
        tm_.tail_repairs++;
        if (timing_) IPO_HIP_CHECK(hipEventRecord(ev0_, s));
        static_assert(kFlagTailBlock == kFlagBail + 1, "one memset clears both");
        IPO_HIP_CHECK(hipMemsetAsync(dFlags_.get() + kFlagBail, 0, 2 * sizeof(int), s));
        TailView tv = tail_view();
        if (verdict_.needs_restore()) launch_tail_restore(pv, tv, tb, s);   // other workgroups of the DEP pass wrote
        ph_begin(s);
        if (tb > 0) launch_tail_colupdate(pv, tv, tb - 1, s);
        ph_end(kPhTail, tb > 0, s);
        // block column tb with the dependent-pivot rule, one round per dependent pivot
        IPO_HIP_CHECK(hipMemsetAsync(dDepI_.get(), 0, 8 * sizeof(int), s));
        // rounds enqueued kDepBatch at a time (a round after the last is a
        // no-op), one host read-back per batch instead of per round; round r
        // writes state copy (r + 1) & 1, so the batch's last round wrote
        // copy (r + kDepBatch) & 1
        constexpr int kDepBatch = 4;
        for (int r = 0;; r += kDepBatch) {
            if (r > kPanelCols + 1) throw std::runtime_error("kkt: dense-tail dependent-pivot rounds did not finish");
            ph_begin(s);
            for (int b = 0; b < kDepBatch; b++)
                launch_tail_dep_round(pv, tv, tb, r + b, dDepSt_.get(), dDepI_.get(), s);
            ph_end(kPhTail, kDepBatch, s);
            IPO_HIP_CHECK(hipMemcpyAsync(hDepDone_, dDepI_.get() + 4 * ((r + kDepBatch) & 1) + 2, sizeof(int),
                                         hipMemcpyDeviceToHost, s));
            IPO_HIP_CHECK(hipStreamSynchronize(s));
            tm_.tail_dep_rounds += kDepBatch;
            if (*hDepDone_) break;
        }
        if (h_.paths.tail_run) {
            launch_tail_from(tb + 1, false);
        } else {
            ph_begin(s);
            for (int t = tb + 1; t < plan_.ntb; t++) launch_tail_step(pv, tail_view(), t, s);
            ph_end(kPhTail, plan_.ntb - tb - 1, s);
        }
        if (finish_pass(true)) break;
        if (!verdict_.tail_only() || verdict_.tail_col() <= tb)   // cannot happen: a later tail column or nothing
            throw std::runtime_error("kkt: dense-tail repair did not advance");
    }
}

// Gather launch of one level (tail < 0) or of the dense tail (group =
// nlevels): every chunk; split units combined by their last-arriving chunk.
int KktDevice::launch_gather(const PlanView& pv, const TailView& tv, int tail, int group, hipStream_t s) {
    const int c0 = h_.ck_ptr[group], c1 = h_.ck_ptr[group + 1];
    if (c1 <= c0) return 0;
    const SlotRec* recs = tail < 0 ? dslot_rec_.get() : dtail_slot_rec_.get();
    // groups whose split units have many chunks sum their partials four
    // at a time (more registers: three waves per SIMD drop to two, which
    // the gathers of the other groups would pay for)
    // developer stamps (IPO_HIP_GATHER_STAMPS=<group>): per workgroup
    // s_memrealtime at start / records / values / MFMA / put / stores
    long long* stq = nullptr;
    if (gst_group_ == group && tail < 0 && h_.ck_kind[group] > 0) {
        if (!dGStamp_.get()) dGStamp_.alloc(1024 * 8);
        stq = dGStamp_.get();
        gst_n_ = c1 - c0;
    }
    if (h_.ck_kind[group] == 2) {
        hipLaunchKernelGGL(k_update_quad, dim3(c1 - c0), dim3(NT), 0, s, pv, tv, recs, dck_u_.get(), dck_b_.get(),
                           dck_e_.get(), dck_part_.get(), c0, stq);
        return 1;
    }
    if (h_.ck_kind[group] == 1) {
        if (h_.ck_wide[group])
        hipLaunchKernelGGL(k_update_flat<4>, dim3(c1 - c0), dim3(NT), 0, s, pv, tv, tail, recs, dck_u_.get(),
                           dck_b_.get(), dck_e_.get(), dck_part_.get(), c0, dPartialTile_.get(), dck_q_.get(),
                           dsp_p0_.get(), dsp_n_.get(), dSplitCnt_.get(), stq);
        else
        hipLaunchKernelGGL(k_update_flat<1>, dim3(c1 - c0), dim3(NT), 0, s, pv, tv, tail, recs, dck_u_.get(),
                           dck_b_.get(), dck_e_.get(), dck_part_.get(), c0, dPartialTile_.get(), dck_q_.get(),
                           dsp_p0_.get(), dsp_n_.get(), dSplitCnt_.get(), stq);
        return 1;
    }
    const int occ = knobs_.update_occ;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(c1 - c0), dim3(NT), 0, s, pv, tv, tail, recs, dck_u_.get(), dck_b_.get(),
                           dck_e_.get(), dck_part_.get(), c0, dPartialTile_.get(), dck_q_.get(), dsp_p0_.get(),
                           dsp_n_.get(), dSplitCnt_.get());
    };
    if (h_.ck_wide[group]) {
        // (four partials in flight spill at 128 and at 168 VGPRs; 3 per CU
        // with 16 spilled measured no faster than 2 per CU)
        go(k_update<4, 1>);
    } else {
        if (occ == 4) go(k_update<1, 4>);
        else go(k_update<1, 1>);
    }
    return 1;
}

hipEvent_t KktDevice::next_event() {
    if (kev_used_ == kev_.size()) {
        hipEvent_t e;
        IPO_HIP_CHECK(hipEventCreate(&e));
        kev_.push_back(e);
    }
    return kev_[kev_used_++];
}

void KktDevice::ph_begin(hipStream_t s) {
    if (!timing_) return;
    mark_b_ = next_event();
    IPO_HIP_CHECK(hipEventRecord(mark_b_, s));
}

void KktDevice::ph_end(int phase, int launches, hipStream_t s) {
    if (!timing_) return;
    hipEvent_t e = next_event();
    IPO_HIP_CHECK(hipEventRecord(e, s));
    marks_.push_back({mark_b_, e, phase, launches});
}

void KktDevice::ph_collect() {
    for (const PhaseMark& mk : marks_) {
        float ms = 0;
        IPO_HIP_CHECK(hipEventElapsedTime(&ms, mk.b, mk.e));
        tm_.phase_ms[mk.phase] += ms;
        tm_.phase_launches[mk.phase] += mk.launches;
    }
    marks_.clear();
    kev_used_ = 0;
}

void KktDevice::launch_q_long(const double* v, double* out) {
    ipo::launch_q_long(q_long_n_, dQLongCols_.get(), dkQ_.get(), diQ_.get(), dQ_.get(), v, out, stream_);
}

void KktDevice::set_long_rows(int row0) {
    if (xch_ || row0 < 0 || row0 >= m_) return;
    long_row0_ = row0;
    dLongAx_.alloc(2 * static_cast<size_t>(m_ - row0));
}

// Refined solves of R systems K [dy; dx] = [fy_r; fx_r] with the current
// factor, in place (ldlt.c:327-425).  Each right-hand side runs the
// reference's own refinement loop (first pass from the right-hand side,
// further passes on the KKT residual while it exceeds 1e-10 (max|b| + 1)
// and halves, the last correction undone if the residual grew); passes of
// both systems share one sweep.  Returns the reference's consistency flag
// of each system in ok[r].
void KktDevice::solve_multi(int R, const double* dE, const double* dD, double* const* dfy, double* const* dfx,
                            int* ok) {
    hipStream_t s = stream_;
    if (timing_) IPO_HIP_CHECK(hipEventRecord(ev0_, s));
    const int m = m_, n = n_, T = T_;
    // the first pass's head and the forward steps before the tail lead: done
    // beside the factorisation (the pre-pass, joined there), or now
    const bool pre_lead = pre_lead_;         // (take_prepass spends it)
    const bool pre = take_prepass(R, dfy, dfx);
    if (!pre && R > 0) enqueue_pass_head(R, dfy, dfx, dPart_.get(), s);
    double maxbc[2] = {0.0, 0.0}, rs[2] = {HUGE_VAL, HUGE_VAL}, rs_old[2] = {HUGE_VAL, HUGE_VAL};
    int pass[2] = {0, 0};
    bool active[2] = {R > 0, R > 1};
    auto zv = [&](int r) { return dZ_.get() + (size_t)r * T; };
    auto dyv = [&](int r) { return dDy_.get() + (size_t)r * m; };
    auto dxv = [&](int r) { return dDx_.get() + (size_t)r * n; };
    auto ryv = [&](int r) { return dRy_.get() + (size_t)r * m; };
    auto rxv = [&](int r) { return dRx_.get() + (size_t)r * n; };
    // the reference's consistency flag is that of each system's last rawsolve
    // (ldlt.c:379, 424): flags are cleared before every sweep, and the sweep's
    // right-hand-side slot q of an active system is read back after it
    int incons[2] = {0, 0};
    while (active[0] || active[1]) {
        const bool first = pass[0] + pass[1] == 0;     // (every system is active in it)
        if (!first) {
            PermJobs J{};
            int na = 0;
            for (int r = 0; r < R; r++)
                if (active[r]) {
                    J.fy[na] = ryv(r);
                    J.fx[na] = rxv(r);
                    J.z[na] = zv(r);
                    na++;
                }
            hipLaunchKernelGGL(k_perm_in2, dim3(ceil_div(T, NT), na), dim3(NT), 0, s, T, m, dperm_.get(), J,
                               dIncons_.get(), sweep_eps());
        }
        eps_cleared_ = true;
        // (the pre-pass ran the tail lead too: IPO_HIP_LEAD_TRAIL)
        const size_t fwd_first = first && pre ? static_cast<size_t>(pre_lead ? h_.sweep.lead_end : h_.sweep.split) : 0;
        if (active[0] && active[1]) rawsolve(zv(0), 2, fwd_first);
        else rawsolve(zv(active[0] ? 0 : 1), 1, fwd_first);
        eps_cleared_ = false;
        int nq = 0;
        {
            PermJobs P{};
            ResJobs J{};
            const int mrow = xch_ ? m - nforced_ : long_row0_ >= 0 ? long_row0_ : m;
            for (int r = 0; r < R; r++) {
                if (!active[r]) continue;
                P.z[nq] = zv(r); P.dy[nq] = dyv(r); P.dx[nq] = dxv(r); P.mode[nq] = pass[r] == 0 ? 0 : 1;
                J.fy[nq] = dfy[r]; J.fx[nq] = dfx[r]; J.dy[nq] = dyv(r); J.dx[nq] = dxv(r);
                J.ry[nq] = ryv(r); J.rx[nq] = rxv(r);
                J.axl[nq] = xch_ ? dLinkAx_.get() + (size_t)r * nforced_
                                 : long_row0_ >= 0 ? dLongAx_.get() + (size_t)r * (m - long_row0_) : nullptr;
                J.qxl[nq] = q_long_n_ > 0 ? dLongQ_.get() + (size_t)r * m : nullptr;
                nq++;
            }
            hipLaunchKernelGGL(k_perm_out2, dim3(ceil_div(T, NT), nq), dim3(NT), 0, s, T, m, diperm_.get(), P);
            for (int q = 0; q < nq; q++) {
                double* axl = const_cast<double*>(J.axl[q]);
                if (xch_) {
                    launch_link_ax(mrow, m, dkAt_.get(), diAt_.get(), dAt_.get(), J.dx[q], axl, s);
                    xsum(axl, nforced_, RedOp::Sum);
                } else if (long_row0_ >= 0) {
                    launch_link_ax(mrow, m, dkAt_.get(), diAt_.get(), dAt_.get(), J.dx[q], axl, s);
                }
                if (q_long_n_ > 0) launch_q_long(J.dy[q], const_cast<double*>(J.qxl[q]));
            }
            hipLaunchKernelGGL(k_kkt_residual2, dim3(kRedBlocks, nq), dim3(kResThreads), 0, s, m, n, dkAt_.get(),
                               diAt_.get(), dAt_.get(), dkA_.get(), diA_.get(), dA_.get(), dE, dD, J, dPart_.get(), mrow,
                               dkQ_.get() ? dkQ_.get() : static_cast<const int*>(nullptr), diQ_.get(), dQ_.get(),
                               static_cast<double>(qmax_), q_long_min());
        }
        // residuals and the consistency flags in one read-back
        if (xch_) {
            hipLaunchKernelGGL(k_finish_reduce, dim3(1), dim3(kRedThreads), 0, s, dPart_.get(), nq, (1u << nq) - 1u,
                               dScal_.get() + kScRes);
            xsum(dScal_.get() + kScRes, nq, RedOp::Max);
            hipLaunchKernelGGL(k_pack_ints, dim3(1), dim3(2), 0, s, dIncons_.get(), 2, dScal_.get() + kScIncons);
        } else {
            hipLaunchKernelGGL(k_finish_reduce_pack, dim3(1), dim3(kRedThreads), 0, s, dPart_.get(), nq,
                               (1u << nq) - 1u, dScal_.get() + kScRes, static_cast<const int*>(dIncons_.get()), 2,
                               dScal_.get() + kScIncons);
        }
        IPO_HIP_CHECK(hipMemcpyAsync(hScal_, dScal_.get(), (first ? kScMaxbc + 2 * R : kScReadLater) * sizeof(double),
                                     hipMemcpyDeviceToHost, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        if (first)
            for (int r = 0; r < R; r++) {
                const double* mb = hScal_ + kScMaxbc + 2 * r;
                maxbc[r] = (mb[0] > mb[1] ? mb[0] : mb[1]) + 1;
            }
        int slot_incons[2];      // of the sweep's right-hand-side slots
        std::memcpy(slot_incons, hScal_ + kScIncons, sizeof(slot_incons));
        const double* res = hScal_ + kScRes;
        int q = 0;
        for (int r = 0; r < R; r++) {
            if (!active[r]) continue;
            incons[r] = slot_incons[q];
            rs_old[r] = rs[r];
            rs[r] = res[q++];
            pass[r]++;
            active[r] = rs[r] > 1.0e-10 * maxbc[r] && rs[r] < rs_old[r] / 2;
        }
    }
    CopyOut co{};
    for (int r = 0; r < R; r++) {
        if (rs[r] > rs_old[r] && pass[r] > 1)
            hipLaunchKernelGGL(k_perm_out, dim3(ceil_div(T, NT)), dim3(NT), 0, s, T, m, diperm_.get(), zv(r), dyv(r),
                               dxv(r), 2);
        co.src[2 * r] = dyv(r); co.dst[2 * r] = dfy[r];
        co.src[2 * r + 1] = dxv(r); co.dst[2 * r + 1] = dfx[r];
    }
    // the solutions back into the callers' vectors: one launch for all
    // 2R copies (four copy-engine calls cost four host round trips)
    co.m = m;
    co.n = n;
    co.R = R;
    if (R > 0 && m + n > 0) hipLaunchKernelGGL(k_copy_out, dim3(ceil_div(R * (m + n), NT)), dim3(NT), 0, s, co);
    if (timing_) {   // otherwise the caller's next read-back orders the copies
        IPO_HIP_CHECK(hipEventRecord(ev1_, s));
        IPO_HIP_CHECK(hipStreamSynchronize(s));
        float ms = 0;
        IPO_HIP_CHECK(hipEventElapsedTime(&ms, ev0_, ev1_));
        tm_.solve_ms += ms;
    }
    tm_.solves += R;
    last_passes_ = pass[0] + pass[1];
    for (int r = 0; r < R; r++) ok[r] = incons[r] ? 0 : 1;
}

// Whether the solve about to start finds its first pass's head and leading
// forward steps done by the last factorisation's pre-pass: one that stood
// (factor_core), for these right-hand sides.  Used or not, it is spent.
bool KktDevice::take_prepass(int R, double* const* dfy, double* const* dfx) {
    bool same = pre_state_ == kPreValid && !timing_ && pre_req_.R == R;
    for (int r = 0; same && r < R; r++) same = pre_req_.dfy[r] == dfy[r] && pre_req_.dfx[r] == dfx[r];
    if (!same) {
        drop_prepass();
        return false;
    }
    pre_state_ = kPreNone;
    pre_used_++;
    if (pre_lead_) lead_used_++;
    pre_lead_ = false;
    return true;
}

int KktDevice::solve(const double* dE, const double* dD, double* dfy, double* dfx) {
    int ok[1];
    solve_multi(1, dE, dD, &dfy, &dfx, ok);
    return ok[0];
}

int KktDevice::solve2(const double* dE, const double* dD, double* dfy1, double* dfx1, double* dfy2, double* dfx2) {
    double* fy[2] = {dfy1, dfy2};
    double* fx[2] = {dfx1, dfx2};
    int ok[2];
    solve_multi(2, dE, dD, fy, fx, ok);
    return ok[0] && ok[1];
}

void KktDevice::download_factor(double* lx, double* d, int* live) const {
    if (lx) dLx_.download(lx, plan_.lx_size, stream_);
    if (d) dDg_.download(d, T_, stream_);
    if (live) dLive_.download(live, T_, stream_);
    IPO_HIP_CHECK(hipStreamSynchronize(stream_));
}

}  // namespace ipo
