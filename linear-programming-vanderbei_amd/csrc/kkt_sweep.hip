// kkt_sweep.hip -- the substitution sweeps of the supernodal LDL' (rawsolve,
// ldlt.c:433-505): every sweep kernel and the KktDevice members that launch
// them.  Factor and refined solve: kkt_device.hip; the layout of Lx and dg
// is described there.  Each section below opens with its own comment.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cstdio>
#include <initializer_list>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "dev_common.h"
#include "kkt_device.h"
#include "kkt_kernels.h"

namespace ipo {

namespace {

// -------------------------------------------------------------- solves
// Every sweep kernel handles R right-hand sides at once (R = 1 or 2; hsd and
// hsdls solve two systems with the same factor per iteration, hsd.c:218-224):
// vector r of a family lives at base + r * stride.  The dependency chain of a
// sweep is the same for both, so the second vector rides along almost free.
//
// One wave solves a unit-lower nc x nc block in place: lane r holds z_r on
// entry and on exit; Ls[r][j] = L(r, j) (zero for j >= r).  Lane r keeps its
// row of L in registers; z_j is broadcast by v_readlane.  A dropped column j
// (mark false) keeps z_j when |z_j| > eps (and the system is flagged
// inconsistent), else z_j = 0 -- ldlt.c:446-470.
// Fast form when every column of the block is live (the common case):
// NS = 16, 32 or 64 >= nc steps with no per-step branch (a step j >= nc
// subtracts L(r, j) z_j = 0 * 0 and changes nothing), so the chain is one
// basic block the compiler can schedule; the same mul-then-subtract per
// entry as the general form (bitwise the same result).
// The lane index, opaque to the optimiser (OPQ solves): a solve inside a
// loop would otherwise have its 64 per-step lane masks hoisted out of the
// loop (128 scalar registers, spilled: the sync-free sweeps, the lead
// sweep).  Outside loops the hoisted masks are cheaper (OPQ = false).
__device__ __forceinline__ int opaque_lane() {
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    return lane;
}
template <int R, int NS, bool OPQ>
__device__ __forceinline__ void tri_lower_live(double (&zr)[R], const double (*Ls)[PC + 1]) {
    const int lane = OPQ ? opaque_lane() : (int)(threadIdx.x & 63);
    double lr[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) lr[j] = Ls[lane][j];
#pragma unroll
    for (int j = 0; j < NS; j++) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double zj = lane_bcast(zr[r], j);
            const double nz = zr[r] - lr[j] * zj;
            zr[r] = lane > j ? nz : zr[r];
        }
    }
}
template <int R, int NS, bool OPQ>
__device__ __forceinline__ void tri_upper_live(double (&zr)[R], const double (*Ls)[PC + 1]) {
    const int lane = OPQ ? opaque_lane() : (int)(threadIdx.x & 63);
    double lc[NS];
#pragma unroll
    for (int j = 0; j < NS; j++) lc[j] = Ls[j][lane];
#pragma unroll
    for (int j = NS - 1; j >= 0; j--) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double zj = lane_bcast(zr[r], j);
            const double nz = zr[r] - lc[j] * zj;
            zr[r] = lane < j ? nz : zr[r];
        }
    }
}

template <int R, bool OPQ = false>
__device__ __forceinline__ void tri_lower(double (&zr)[R], const double (*Ls)[PC + 1], const int* lv, int nc,
                                          const double (&eps)[R], int (&bad)[R]) {
    const int lane = OPQ ? opaque_lane() : (int)(threadIdx.x & 63);
    const uint64_t lm = __ballot(lane < nc && lv[lane]);
    if (lm == (nc >= 64 ? ~0ull : (1ull << nc) - 1ull)) {     // every column live (wave-uniform)
        if (nc <= 16) tri_lower_live<R, 16, OPQ>(zr, Ls);
        else if (nc <= 32) tri_lower_live<R, 32, OPQ>(zr, Ls);
        else tri_lower_live<R, 64, OPQ>(zr, Ls);
        return;
    }
    double lr[PC];
#pragma unroll
    for (int j = 0; j < PC; j++) lr[j] = lane < nc ? Ls[lane][j] : 0.0;
#pragma unroll
    for (int j = 0; j < PC; j++) {
        if (j < nc) {
            const bool alive = (lm >> j) & 1ull;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (!alive && lane == j) {
                    if (fabs(zr[r]) > eps[r]) bad[r] = 1;
                    else zr[r] = 0.0;
                }
                const double zj = lane_bcast(zr[r], j);
                if (alive && lane > j) zr[r] -= lr[j] * zj;
            }
        }
    }
}

// unit-upper (L11') counterpart; Ls[j][r] = L(j, r) (zero for r >= j)
template <int R, bool OPQ = false>
__device__ __forceinline__ void tri_upper(double (&zr)[R], const double (*Ls)[PC + 1], const int* lv, int nc,
                                          const double (&eps)[R], int (&bad)[R]) {
    const int lane = OPQ ? opaque_lane() : (int)(threadIdx.x & 63);
    const uint64_t lm = __ballot(lane < nc && lv[lane]);
    if (lm == (nc >= 64 ? ~0ull : (1ull << nc) - 1ull)) {     // every column live (wave-uniform)
        if (nc <= 16) tri_upper_live<R, 16, OPQ>(zr, Ls);
        else if (nc <= 32) tri_upper_live<R, 32, OPQ>(zr, Ls);
        else tri_upper_live<R, 64, OPQ>(zr, Ls);
        return;
    }
    double lc[PC];
#pragma unroll
    for (int j = 0; j < PC; j++) lc[j] = j < nc ? Ls[j][lane] : 0.0;
#pragma unroll
    for (int j = PC - 1; j >= 0; j--) {
        if (j < nc) {
            const bool alive = (lm >> j) & 1ull;
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (!alive && lane == j) {
                    if (fabs(zr[r]) > eps[r]) bad[r] = 1;
                    else zr[r] = 0.0;
                }
                const double zj = lane_bcast(zr[r], j);
                if (alive && lane < j) zr[r] -= lc[j] * zj;
            }
        }
    }
}

// Column sums of a wave's 16 (x R) per-lane partials without 16 R serial
// chains of cross-lane permutes: each wave writes its partials to LDS
// scratch (rows padded to PC + 1 doubles: conflict-free column writes and
// row reads), then one thread per (right-hand side, column) redoes
// wave_sum's shfl_down tree (v[l] += v[l + o], o = 32 .. 1, result in lane
// 0) on its row -- the same adds in the same order, so bitwise the same.
// Scratch: R * PC * (PC + 1) doubles; a __syncthreads between the two.
template <int R>
__device__ __forceinline__ void colsum_put(double* red, const double (&v)[R][16], int kq, int nq, int lane) {
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (q < nq) red[(size_t)(r * PC + kq + q) * (PC + 1) + lane] = v[r][q];
}
__device__ __forceinline__ double colsum_tree(const double* red, int r, int c) {
    const double* __restrict__ x = red + (size_t)(r * PC + c) * (PC + 1);
    double s[32];
#pragma unroll
    for (int l = 0; l < 32; l++) s[l] = x[l] + x[l + 32];
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int l = 0; l < o; l++) s[l] += s[l + o];
    return s[0];
}

template <int R>
__device__ __forceinline__ void flag_bad(const PlanView& p, const int (&bad)[R]) {
#pragma unroll
    for (int r = 0; r < R; r++)
        if (bad[r]) atomicOr(&p.incons[r], 1);
}

template <int R>
__device__ __forceinline__ void load_eps(const double* epsp, double (&eps)[R]) {
#pragma unroll
    for (int r = 0; r < R; r++) eps[r] = epsp[r];
}

// D^{-1} with the dropped-column rule (ldlt.c:473-480)
__device__ __forceinline__ double dscale_rule(const PlanView& p, int v, double zv, double eps, int& bad) {
    if (p.live[v]) return zv / p.dg[v];
    if (fabs(zv) > eps) bad = 1;
    else zv = 0.0;
    return zv;
}

// Stage L11 of a panel (ld = h) from the upper-triangle slot image:
// Ls[r][j] = L(r, j) for j < r, 0 elsewhere.  Each wave issues all its
// loads before the first LDS store (addresses clamped in bounds).
// Waves wv of nw (default: the whole workgroup) share the loads.
__device__ __forceinline__ void stage_l11(const double* panel, size_t ld, int nc, double (*Ls)[PC + 1], int wv,
                                          int nw) {
    const int lane = threadIdx.x & 63;
    for (int r0 = wv; r0 < PC; r0 += 16 * nw) {
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = r0 + q * nw;
            const bool ok = r < nc && lane < r;
            t[q] = panel[ok ? lane + (size_t)r * ld : 0];
            t[q] = ok ? t[q] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = r0 + q * nw;
            if (r < PC) Ls[r][lane] = t[q];
        }
    }
}
__device__ __forceinline__ void stage_l11(const double* panel, size_t ld, int nc, double (*Ls)[PC + 1]) {
    stage_l11(panel, ld, nc, Ls, threadIdx.x >> 6, blockDim.x >> 6);
}

// Vector families of a sweep: z (K entries each) and the forward update
// values ybuf (one per row of every R_s).
struct SweepVecs {
    double* z;
    size_t zs;          // stride between right-hand sides
    double* y;
    size_t ys;
};

// Forward, diagonal part of supernode s: subtract the y values of solved
// descendants from its rows, solve L11.  Leaves z_s in zl[r] and in z.
// 4 threads per row; partial sums combined as (p0 + p1) + (p2 + p3).
// per-item wall-clock stamps of the last forward sync-free sweep (developer
// build with -DIPO_SF_STAMPS; dumped by ~KktDevice)
#ifdef IPO_SF_STAMPS
__device__ long long g_sfst[1 << 15][10];
#define SF_STAMP(it, slot) do { if (threadIdx.x == 0 && (it) >= 0 && (it) < (1 << 15)) g_sfst[it][slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define SF_NOTE(it, slot, v) do { if (threadIdx.x == 0 && (it) >= 0 && (it) < (1 << 15)) g_sfst[it][slot] = (v); } while (0)
#else
#define SF_STAMP(it, slot) do {} while (0)
#define SF_NOTE(it, slot, v) do {} while (0)
#endif

// sidx != nullptr: the supernode's update-list indices, yrow_idx[yrow_ptr[c0]
// ..], already staged in LDS by the caller (before its hand-off wait), so
// only the value loads remain on the chain -- sixteen in flight per thread.
template <int R, bool SC = false, bool STAGED = false>
__device__ void fwd_diag(const PlanView& p, int s, const int* __restrict__ yrow_ptr, const int* __restrict__ yrow_idx,
                         const SweepVecs& V, const double (&eps)[R], double (*zl)[PC], double (*Ls)[PC + 1], int* lv,
                         const int* sidx = nullptr, int stamp_it = -1, const int* sptr = nullptr,
                         double* zout = nullptr, size_t zos = 0) {
    const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
    const int h = nc + (p.rowptr[s + 1] - p.rowptr[s]);
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    if (!STAGED) {              // else the caller staged L11 and the marks already
        stage_l11(p.Lx + p.off[s], h, nc, Ls);
        if (tid < nc) lv[tid] = p.live[c0 + tid];
    }
    // P threads per row (P = 256 / nc rounded down to a power of two, 4..64):
    // part q sums the entries q, q + P, ... of the row's list in list order
    // (sixteen loads in flight), then a fixed xor-butterfly combines the P
    // partial sums -- the same order in every kernel that calls this.
    const int P = nc > 32 ? 4 : nc > 16 ? 8 : nc > 8 ? 16 : nc > 4 ? 32 : 64;
    // sptr: the rows' list bounds yrow_ptr[c0 .. c0 + nc], staged in LDS by the caller
    const int ebase = sidx ? (sptr ? sptr[0] : yrow_ptr[c0]) : 0;
    // list index e: the staged LDS copy or the global list (no pointer
    // arithmetic across address spaces)
    auto lidx = [&](int e) { return sidx ? sidx[e - ebase] : yrow_idx[e]; };
    for (int base = 0; base < nc; base += blockDim.x / P) {
        const int k = base + tid / P, part = tid & (P - 1);
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0.0;
        if (k < nc) {
            const int v = c0 + k;
            const int e1 = sptr ? sptr[k + 1] : yrow_ptr[v + 1];
            int e = (sptr ? sptr[k] : yrow_ptr[v]) + part;
#ifdef IPO_SF_STAMPS
            if (tid == 0 && stamp_it >= 0) { g_sfst[stamp_it][9] = e1 + e; SF_STAMP(stamp_it, 7); }
#endif
            for (; e + 31 * P < e1; e += 32 * P) {     // 32 loads in flight per right-hand side
                int ix[32];
#pragma unroll
                for (int u = 0; u < 32; u++) ix[u] = lidx(e + u * P);
                double yv[R][32];
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int u = 0; u < 32; u++) yv[r][u] = ld_h<SC>(V.y + r * V.ys + ix[u]);
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int u = 0; u < 32; u++) acc[r] += yv[r][u];
            }
            for (; e + 15 * P < e1; e += 16 * P) {
                int ix[16];
#pragma unroll
                for (int u = 0; u < 16; u++) ix[u] = lidx(e + u * P);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const double* yb = V.y + r * V.ys;
                    double yv[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) yv[u] = ld_h<SC>(yb + ix[u]);
#pragma unroll
                    for (int u = 0; u < 16; u++) acc[r] += yv[u];
                }
            }
            for (; e + 3 * P < e1; e += 4 * P) {
                const int i0 = lidx(e), i1 = lidx(e + P), i2 = lidx(e + 2 * P), i3 = lidx(e + 3 * P);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const double* yb = V.y + r * V.ys;
                    const double y0 = ld_h<SC>(yb + i0), y1 = ld_h<SC>(yb + i1), y2 = ld_h<SC>(yb + i2),
                                 y3 = ld_h<SC>(yb + i3);
                    acc[r] += y0;
                    acc[r] += y1;
                    acc[r] += y2;
                    acc[r] += y3;
                }
            }
            for (; e < e1; e += P) {
                const int i0 = lidx(e);
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] += ld_h<SC>(V.y + r * V.ys + i0);
            }
        }
#ifdef IPO_SF_STAMPS
        if (tid == 0 && stamp_it >= 0) { g_sfst[stamp_it][9] += (long long)acc[0]; SF_STAMP(stamp_it, 8); }
#endif
#pragma unroll
        for (int r = 0; r < R; r++) {
            double pr = acc[r];
            for (int o = 1; o < P; o <<= 1) {
                const double ot = __shfl_xor(pr, o, 64);
                pr = (part & o) ? ot + pr : pr + ot;
            }
            if (part == 0 && k < nc) zl[r][k] = V.z[r * V.zs + c0 + k] - pr;
        }
    }
    __syncthreads();
    SF_STAMP(stamp_it, 5);
    if (wv < R) {                 // wave r solves right-hand side r (independent chains)
        const int r = wv;
        int bad[1] = {};
        double zr[1] = {lane < nc ? zl[r][lane] : 0.0};
        const double e1[1] = {r == 0 ? eps[0] : eps[R - 1]};
        tri_lower<1, true>(zr, Ls, lv, nc, e1, bad);
        if (lane < nc) {
            // zout: z_s goes to a mirror instead (the chunk items of one
            // supernode each solve it and must all read its right-hand side)
            if (zout) sc1_store(zout + r * zos + lane, zr[0]);
            else V.z[r * V.zs + c0 + lane] = zr[0];
            zl[r][lane] = zr[0];
        }
        if (bad[0]) atomicOr(&p.incons[r], 1);
    }
    __syncthreads();
}

// Forward, one level of small supernodes per launch, one workgroup each:
// diagonal part, then y_s = L21 z_s for the ancestors (one row per thread).
// D^{-1} is applied at the start of the backward sweep.
template <int R>
__device__ __forceinline__ void forward_body(const PlanView& p, const int* __restrict__ level_sups, int q0,
                                             const int* __restrict__ yrow_ptr, const int* __restrict__ yrow_idx,
                                             const SweepVecs& V, const double* __restrict__ epsp, int bid) {
    __shared__ double zl[R][PC];
    __shared__ double Ls[PC][PC + 1];
    __shared__ int lv[PC];
    double eps[R];
    load_eps<R>(epsp, eps);
    const int s = level_sups[q0 + bid];
    fwd_diag<R>(p, s, yrow_ptr, yrow_idx, V, eps, zl, Ls, lv);
    const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
    const int hb = p.rowptr[s + 1] - p.rowptr[s], h = nc + hb;
    const double* panel = p.Lx + p.off[s];
    for (int i = threadIdx.x; i < hb; i += NT) {
        const double* __restrict__ row = panel + nc + i;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0.0;
#pragma unroll 8
        for (int k = 0; k < nc; k++) {
            const double l = row[(size_t)k * h];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] += l * zl[r][k];
        }
#pragma unroll
        for (int r = 0; r < R; r++) V.y[r * V.ys + p.ybase[s] + i] = acc[r];
    }
}

template <int R>
__global__ void __launch_bounds__(NT)
k_forward(PlanView p, const int* __restrict__ level_sups, int q0, const int* __restrict__ yrow_ptr,
          const int* __restrict__ yrow_idx, SweepVecs V, const double* __restrict__ epsp) {
    forward_body<R>(p, level_sups, q0, yrow_ptr, yrow_idx, V, epsp, blockIdx.x);
}

// Single-column supernodes with at most 64 rows below (the bulk of the
// bottom level: one per x-node of a large LP, 10^6 on configs[3]), one wave
// each, four per workgroup -- k_forward / k_backward spend a 256-thread
// workgroup, an L11 staging and two barriers on each.  The same operations
// in the same order as those kernels' nc = 1 case (the update list summed
// by 64 parts, part q taking entries q, q + 64, ... in list order, the
// parts combined by the xor butterfly; the backward products summed by
// wave_sum), so bitwise the same sweep.
template <int R>
__device__ __forceinline__ void fwd_leaf_body(const PlanView& p, const int* __restrict__ sups, int q0, int cnt,
                                              const int* __restrict__ yrow_ptr, const int* __restrict__ yrow_idx,
                                              const SweepVecs& V, const double* __restrict__ epsp, int bid) {
    const int w = bid * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= cnt) return;
    const int s = sups[q0 + w];
    const int c0 = p.col0[s], hb = p.rowptr[s + 1] - p.rowptr[s];
    double pr[R];
#pragma unroll
    for (int r = 0; r < R; r++) pr[r] = 0.0;
    for (int e = yrow_ptr[c0] + lane; e < yrow_ptr[c0 + 1]; e += 64) {
        const int ix = yrow_idx[e];
#pragma unroll
        for (int r = 0; r < R; r++) pr[r] += V.y[r * V.ys + ix];
    }
    double z[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        for (int o = 1; o < 64; o <<= 1) {
            const double ot = __shfl_xor(pr[r], o, 64);
            pr[r] = (lane & o) ? ot + pr[r] : pr[r] + ot;
        }
        z[r] = __shfl(V.z[r * V.zs + c0] - pr[r], 0, 64);
    }
    if (!p.live[c0]) {          // dropped column (ldlt.c:446-470)
        double eps[R];
        load_eps<R>(epsp, eps);
        int bad[R] = {};
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (fabs(z[r]) > eps[r]) bad[r] = 1;
            else z[r] = 0.0;
        }
        if (lane == 0) flag_bad<R>(p, bad);
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; r++) V.z[r * V.zs + c0] = z[r];
    }
    if (lane < hb) {
        const double l = p.Lx[p.off[s] + 1 + lane];
#pragma unroll
        for (int r = 0; r < R; r++) {
            double acc = 0.0;
            acc += l * z[r];
            V.y[r * V.ys + p.ybase[s] + lane] = acc;
        }
    }
}

template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_leaf(PlanView p, const int* __restrict__ sups, int q0, int cnt, const int* __restrict__ yrow_ptr,
           const int* __restrict__ yrow_idx, SweepVecs V, const double* __restrict__ epsp) {
    fwd_leaf_body<R>(p, sups, q0, cnt, yrow_ptr, yrow_idx, V, epsp, blockIdx.x);
}

// One launch per level for a level's leaves and its other supernodes
// (workgroups [0, nlb): four leaves each, fwd_leaf_body; the rest one
// supernode each, forward_body) -- the two launches' work in one launch: the
// solve phase's launches are host-bound (the device idles 4-13 us between
// them), so every launch saved is time saved.
template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_level(PlanView p, const int* __restrict__ sups, int q0, int nl, int nlb, const int* __restrict__ yrow_ptr,
            const int* __restrict__ yrow_idx, SweepVecs V, const double* __restrict__ epsp) {
    if (static_cast<int>(blockIdx.x) < nlb) fwd_leaf_body<R>(p, sups, q0, nl, yrow_ptr, yrow_idx, V, epsp, blockIdx.x);
    else forward_body<R>(p, sups, q0 + nl, yrow_ptr, yrow_idx, V, epsp, blockIdx.x - nlb);
}

template <int R>
__device__ __forceinline__ void bwd_leaf_body(const PlanView& p, const int* __restrict__ sups, int q0, int cnt,
                                              const SweepVecs& V, const double* __restrict__ epsp, int bid) {
    const int w = bid * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w >= cnt) return;
    const int s = sups[q0 + w];
    const int c0 = p.col0[s], hb = p.rowptr[s + 1] - p.rowptr[s];
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    if (lane < hb) {
        const int ri = p.rows[p.rowptr[s] + lane];
        const double t = p.Lx[p.off[s] + 1 + lane];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] += t * V.z[r * V.zs + ri];
    }
    double eps[R];
    load_eps<R>(epsp, eps);
    int bad[R] = {};
#pragma unroll
    for (int r = 0; r < R; r++) {
        const double xs = wave_sum(acc[r]);
        if (lane == 0) {
            double zr = dscale_rule(p, c0, V.z[r * V.zs + c0], eps[r], bad[r]) - xs;
            if (!p.live[c0]) {
                if (fabs(zr) > eps[r]) bad[r] = 1;
                else zr = 0.0;
            }
            V.z[r * V.zs + c0] = zr;
        }
    }
    if (lane == 0) flag_bad<R>(p, bad);
}

template <int R>
__global__ void __launch_bounds__(NT)
k_bwd_leaf(PlanView p, const int* __restrict__ sups, int q0, int cnt, SweepVecs V, const double* __restrict__ epsp) {
    bwd_leaf_body<R>(p, sups, q0, cnt, V, epsp, blockIdx.x);
}

// Small leaves (<= 8 rows below, <= 8 update-list entries: the x-node
// leaves of a large LP) eight to a wave, lanes 8q .. 8q + 7 for leaf q.
// k_fwd_leaf's butterfly over 64 lanes, with entry e in lane e, reduces to
// the three in-group stages followed by adds of +0.0 from the empty lanes
// (one `+ 0.0`: further ones change nothing); k_bwd_leaf's wave_sum reaches
// lane 0 through lanes 0-7 the same way (three adds of +0.0, then the
// row-down steps 4, 2, 1).  Bitwise the one-wave kernels.

template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_leaf8(PlanView p, const int* __restrict__ sups, int q0, int cnt, const int* __restrict__ yrow_ptr,
            const int* __restrict__ yrow_idx, SweepVecs V, const double* __restrict__ epsp) {
    const int w = (blockIdx.x * NT + threadIdx.x) / kSmallLeaf, lq = threadIdx.x & (kSmallLeaf - 1);
    if (w >= cnt) return;          // whole groups leave together
    const int s = sups[q0 + w];
    const int c0 = p.col0[s], hb = p.rowptr[s + 1] - p.rowptr[s];
    const int e0 = yrow_ptr[c0], e1 = yrow_ptr[c0 + 1];
    double pr[R];
#pragma unroll
    for (int r = 0; r < R; r++) pr[r] = 0.0;
    if (e0 + lq < e1) {
        const int ix = yrow_idx[e0 + lq];
#pragma unroll
        for (int r = 0; r < R; r++) pr[r] += V.y[r * V.ys + ix];
    }
    double z[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        for (int o = 1; o < kSmallLeaf; o <<= 1) {
            const double ot = __shfl_xor(pr[r], o, kSmallLeaf);
            pr[r] = (lq & o) ? ot + pr[r] : pr[r] + ot;
        }
        pr[r] = pr[r] + 0.0;
        z[r] = __shfl(V.z[r * V.zs + c0] - pr[r], 0, kSmallLeaf);
    }
    if (!p.live[c0]) {          // dropped column (ldlt.c:446-470)
        double eps[R];
        load_eps<R>(epsp, eps);
        int bad[R] = {};
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (fabs(z[r]) > eps[r]) bad[r] = 1;
            else z[r] = 0.0;
        }
        if (lq == 0) flag_bad<R>(p, bad);
    }
    if (lq == 0) {
#pragma unroll
        for (int r = 0; r < R; r++) V.z[r * V.zs + c0] = z[r];
    }
    if (lq < hb) {
        const double l = p.Lx[p.off[s] + 1 + lq];
#pragma unroll
        for (int r = 0; r < R; r++) {
            double acc = 0.0;
            acc += l * z[r];
            V.y[r * V.ys + p.ybase[s] + lq] = acc;
        }
    }
}

template <int R>
__global__ void __launch_bounds__(NT)
k_bwd_leaf8(PlanView p, const int* __restrict__ sups, int q0, int cnt, SweepVecs V, const double* __restrict__ epsp) {
    const int w = (blockIdx.x * NT + threadIdx.x) / kSmallLeaf, lq = threadIdx.x & (kSmallLeaf - 1);
    if (w >= cnt) return;
    const int s = sups[q0 + w];
    const int c0 = p.col0[s], hb = p.rowptr[s + 1] - p.rowptr[s];
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    if (lq < hb) {
        const int ri = p.rows[p.rowptr[s] + lq];
        const double t = p.Lx[p.off[s] + 1 + lq];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] += t * V.z[r * V.zs + ri];
    }
    double eps[R];
    load_eps<R>(epsp, eps);
    int bad[R] = {};
#pragma unroll
    for (int r = 0; r < R; r++) {
        double v = acc[r] + 0.0;                      // wave_sum's steps from lanes 32+, 16+, 8+
        v += __shfl_down(v, 4, kSmallLeaf);
        v += __shfl_down(v, 2, kSmallLeaf);
        v += __shfl_down(v, 1, kSmallLeaf);
        if (lq == 0) {
            double zr = dscale_rule(p, c0, V.z[r * V.zs + c0], eps[r], bad[r]) - v;
            if (!p.live[c0]) {
                if (fabs(zr) > eps[r]) bad[r] = 1;
                else zr = 0.0;
            }
            V.z[r * V.zs + c0] = zr;
        }
    }
    if (lq == 0) flag_bad<R>(p, bad);
}

// Forward for levels with large panels, part 1: diagonal parts only.
template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_diag(PlanView p, const int* __restrict__ level_sups, int q0, const int* __restrict__ yrow_ptr,
           const int* __restrict__ yrow_idx, SweepVecs V, const double* __restrict__ epsp) {
    __shared__ double zl[R][PC];
    __shared__ double Ls[PC][PC + 1];
    __shared__ int lv[PC];
    double eps[R];
    load_eps<R>(epsp, eps);
    fwd_diag<R>(p, level_sups[q0 + blockIdx.x], yrow_ptr, yrow_idx, V, eps, zl, Ls, lv);
}

// part 2: y = L21 z_s over one 64-row chunk of R_s; wave w takes columns
// 16w..16w+15, the four partial sums are added in wave order.
template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_gemv(PlanView p, const int* __restrict__ chunk_sup, const int* __restrict__ chunk_r0, int cb, SweepVecs V) {
    __shared__ double zs[R][PC];
    __shared__ double red[R][4][64];
    const int c = cb + blockIdx.x;
    const int s = chunk_sup[c], r0 = chunk_r0[c];
    const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
    const int hb = p.rowptr[s + 1] - p.rowptr[s], h = nc + hb;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid < nc) {
#pragma unroll
        for (int r = 0; r < R; r++) zs[r][tid] = V.z[r * V.zs + c0 + tid];
    }
    __syncthreads();
    const int i = r0 + lane, kq = wv * 16, nq = min(16, nc - kq);
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    if (i < hb && nq > 0) {
        const double* __restrict__ row = p.Lx + p.off[s] + nc + i + (size_t)kq * h;
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = row[(size_t)min(q, nq - 1) * h];
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (q < nq) {
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] += t[q] * zs[r][kq + q];
            }
    }
#pragma unroll
    for (int r = 0; r < R; r++) red[r][wv][lane] = acc[r];
    __syncthreads();
    if (wv == 0 && i < hb) {
#pragma unroll
        for (int r = 0; r < R; r++)
            V.y[r * V.ys + p.ybase[s] + i] = ((red[r][0][lane] + red[r][1][lane]) + red[r][2][lane]) + red[r][3][lane];
    }
}

// Backward, one level of small supernodes per launch, one workgroup each:
// z_s = D^{-1} z_s - L21' z_R, then L11'.  Wave w owns columns 16w..16w+15,
// lanes stride the rows (coalesced column reads).
template <int R>
__device__ __forceinline__ void backward_body(const PlanView& p, const int* __restrict__ level_sups, int q0,
                                              const SweepVecs& V, const double* __restrict__ epsp, int bid) {
    __shared__ double xs[R][PC];
    __shared__ double Ls[PC][PC + 1];     // Ls[j][r] = L(j, r)
    __shared__ int lv[PC];
    const int s = level_sups[q0 + bid];
    const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
    const int hb = p.rowptr[s + 1] - p.rowptr[s];
    const int h = nc + hb;
    const double* panel = p.Lx + p.off[s];
    const int* __restrict__ rows = p.rows + p.rowptr[s];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    stage_l11(panel, h, nc, Ls);
    if (tid < nc) lv[tid] = p.live[c0 + tid];
    const int kq = wv * 16, nq = min(16, nc - kq);
    if (nq > 0) {
        double acc[R][16];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[r][q] = 0.0;
        for (int i = lane; i < hb; i += 64) {
            const int ri = rows[i];
            double zi[R];
#pragma unroll
            for (int r = 0; r < R; r++) zi[r] = V.z[r * V.zs + ri];
            const double* __restrict__ col = panel + nc + i + (size_t)kq * h;
            double t[16];
#pragma unroll
            for (int q = 0; q < 16; q++) t[q] = col[(size_t)min(q, nq - 1) * h];
#pragma unroll
            for (int q = 0; q < 16; q++)
                if (q < nq) {
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r][q] += t[q] * zi[r];
                }
        }
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int q = 0; q < 16; q++) {
                if (q >= nq) break;           // columns of the wave beyond nc: no reduction
                const double t = wave_sum(acc[r][q]);
                if (lane == 0) xs[r][kq + q] = t;
            }
    }
    __syncthreads();
    if (wv >= R) return;
    // wave r solves right-hand side r (independent chains, one wave each)
    const int r = wv;
    const double e1[1] = {epsp[r]};
    int bad[1] = {};
    double zr[1];
    zr[0] = lane < nc ? dscale_rule(p, c0 + lane, V.z[r * V.zs + c0 + lane], e1[0], bad[0]) - xs[r][lane] : 0.0;
    tri_upper<1>(zr, Ls, lv, nc, e1, bad);
    if (lane < nc) V.z[r * V.zs + c0 + lane] = zr[0];
    if (bad[0]) atomicOr(&p.incons[r], 1);
}

template <int R>
__global__ void __launch_bounds__(NT)
k_backward(PlanView p, const int* __restrict__ level_sups, int q0, SweepVecs V, const double* __restrict__ epsp) {
    backward_body<R>(p, level_sups, q0, V, epsp, blockIdx.x);
}

// k_fwd_level's backward counterpart
template <int R>
__global__ void __launch_bounds__(NT)
k_bwd_level(PlanView p, const int* __restrict__ sups, int q0, int nl, int nlb, SweepVecs V,
            const double* __restrict__ epsp) {
    if (static_cast<int>(blockIdx.x) < nlb) bwd_leaf_body<R>(p, sups, q0, nl, V, epsp, blockIdx.x);
    else backward_body<R>(p, sups, q0 + nl, V, epsp, blockIdx.x - nlb);
}

// Backward for levels with large panels, part 1: per 64-row chunk of R_s,
// part[c][k] = sum over the chunk's rows of L(row, k) z_row.
template <int R>
__global__ void __launch_bounds__(NT)
k_bwd_partial(PlanView p, const int* __restrict__ chunk_sup, const int* __restrict__ chunk_r0, int cb, SweepVecs V,
              double* __restrict__ part, size_t ps) {
    const int c = cb + blockIdx.x;
    const int s = chunk_sup[c], r0 = chunk_r0[c];
    const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
    const int hb = p.rowptr[s + 1] - p.rowptr[s], h = nc + hb;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int kq = wv * 16, nq = min(16, nc - kq);
    if (nq <= 0) return;
    const int i = r0 + lane;
    const bool okr = i < hb;
    const int ic = okr ? i : 0;
    const int ri = p.rows[p.rowptr[s] + ic];
    double zi[R];
#pragma unroll
    for (int r = 0; r < R; r++) zi[r] = V.z[r * V.zs + ri];
    const double* __restrict__ col = p.Lx + p.off[s] + nc + ic + (size_t)kq * h;
    double t[16];
#pragma unroll
    for (int q = 0; q < 16; q++) t[q] = col[(size_t)min(q, nq - 1) * h];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int q = 0; q < 16; q++) {
            if (q >= nq) break;
            const double v = wave_sum(okr ? t[q] * zi[r] : 0.0);
            if (lane == 0) part[r * ps + (size_t)c * PC + kq + q] = v;
        }
}

// part 2: sum the chunks of each supernode (wave w: chunks w, w+4, ...; the
// four partials added in wave order), then D^{-1} and L11'.
template <int R>
__global__ void __launch_bounds__(NT)
k_bwd_finish(PlanView p, const int* __restrict__ level_sups, int q0, const int* __restrict__ sup_chunk0,
             const double* __restrict__ part, size_t ps, SweepVecs V, const double* __restrict__ epsp) {
    __shared__ double Ls[PC][PC + 1];
    __shared__ int lv[PC];
    __shared__ double xs[R][4][PC];
    const int s = level_sups[q0 + blockIdx.x];
    const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
    const int hb = p.rowptr[s + 1] - p.rowptr[s], h = nc + hb;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    stage_l11(p.Lx + p.off[s], h, nc, Ls);
    if (tid < nc) lv[tid] = p.live[c0 + tid];
    {
        const int cf = sup_chunk0[s], nch = (hb + 63) / 64;
        double x[R];
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = 0.0;
        if (lane < nc)
            for (int c = wv; c < nch; c += 4) {
#pragma unroll
                for (int r = 0; r < R; r++) x[r] += part[r * ps + (size_t)(cf + c) * PC + lane];
            }
#pragma unroll
        for (int r = 0; r < R; r++) xs[r][wv][lane] = x[r];
    }
    __syncthreads();
    if (wv >= R) return;
    // wave r solves right-hand side r (independent chains, one wave each)
    const int r = wv;
    const double e1[1] = {epsp[r]};
    int bad[1] = {};
    double zr[1];
    zr[0] = lane < nc ? dscale_rule(p, c0 + lane, V.z[r * V.zs + c0 + lane], e1[0], bad[0]) -
                            (((xs[r][0][lane] + xs[r][1][lane]) + xs[r][2][lane]) + xs[r][3][lane])
                      : 0.0;
    tri_upper<1>(zr, Ls, lv, nc, e1, bad);
    if (lane < nc) V.z[r * V.zs + c0 + lane] = zr[0];
    if (bad[0]) atomicOr(&p.incons[r], 1);
}

// ---------------------------------------------------- dense-tail solves
// forward, part 1: tail rows subtract the y values the sparse panels left
template <int R>
__global__ void __launch_bounds__(NT)
k_tail_gather(TailView tv, const int* __restrict__ yrow_ptr, const int* __restrict__ yrow_idx, SweepVecs V) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blockIdx.x * 4 + wv;
    if (i >= tv.nt) return;
    const int v = tv.tc + i;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    for (int e = yrow_ptr[v] + lane; e < yrow_ptr[v + 1]; e += 64) {
        const int i0 = yrow_idx[e];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] += V.y[r * V.ys + i0];
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        const double a = wave_sum(acc[r]);
        if (lane == 0) V.z[r * V.zs + v] = V.z[r * V.zs + v] - a;
    }
}

// Per-block fallbacks for very large dense tails (ntb > kChainMaxBlocks),
// one right-hand side.  forward, part 2, block kb: every workgroup solves
// the block's L11 in wave 0 (identical arithmetic, identical results;
// workgroup 0 stores it), then updates 64 rows below it.
__global__ void __launch_bounds__(NT)
k_tail_fwd(PlanView p, TailView tv, int kb, double* __restrict__ z, const double* __restrict__ epsp) {
    __shared__ double Ls[PC][PC + 1];
    __shared__ double zb[PC];
    __shared__ int lv[PC];
    __shared__ double red[4][64];
    const int nt = tv.nt, tc = tv.tc, k0 = kb * PC, nc = min(PC, nt - k0);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    stage_l11(tv.S + k0 + (size_t)k0 * nt, nt, nc, Ls);
    if (tid < nc) lv[tid] = p.live[tc + k0 + tid];
    __syncthreads();
    if (wv == 0) {
        int bad[1] = {0};
        double eps[1] = {*epsp};
        double zr[1] = {lane < nc ? z[tc + k0 + lane] : 0.0};
        tri_lower<1>(zr, Ls, lv, nc, eps, bad);
        if (lane < nc) zb[lane] = zr[0];
        if (blockIdx.x == 0) {
            if (lane < nc) z[tc + k0 + lane] = zr[0];
            flag_bad<1>(p, bad);
        }
    }
    __syncthreads();
    const int r = k0 + nc + blockIdx.x * 64 + lane;
    const int kq = wv * 16, nq = min(16, nc - kq);
    double acc = 0.0;
    if (r < nt && nq > 0) {
        const double* __restrict__ row = tv.S + r + (size_t)(k0 + kq) * nt;
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = row[(size_t)min(q, nq - 1) * nt];
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (q < nq) acc += t[q] * zb[kq + q];
    }
    red[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && r < nt) z[tc + r] = z[tc + r] - (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

// backward, part 1: D^{-1} on the tail with the dropped-column rule
__global__ void __launch_bounds__(NT)
k_tail_dscale(PlanView p, TailView tv, double* __restrict__ z, const double* __restrict__ epsp) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= tv.nt) return;
    const int v = tv.tc + i;
    int bad[1] = {0};
    z[v] = dscale_rule(p, v, z[v], *epsp, bad[0]);
    flag_bad<1>(p, bad);
}

// backward, part 2, block kb: L11' solve (every workgroup, workgroup 0
// stores), then 64 columns j < k0 left of it.
__global__ void __launch_bounds__(NT)
k_tail_bwd(PlanView p, TailView tv, int kb, double* __restrict__ z, const double* __restrict__ epsp) {
    __shared__ double Ls[PC][PC + 1];     // Ls[j][r] = L(j, r)
    __shared__ double zb[PC];
    __shared__ int lv[PC];
    __shared__ double red[4][64];
    const int nt = tv.nt, tc = tv.tc, k0 = kb * PC, nc = min(PC, nt - k0);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    stage_l11(tv.S + k0 + (size_t)k0 * nt, nt, nc, Ls);
    if (tid < nc) lv[tid] = p.live[tc + k0 + tid];
    __syncthreads();
    if (wv == 0) {
        int bad[1] = {0};
        double eps[1] = {*epsp};
        double zr[1] = {lane < nc ? z[tc + k0 + lane] : 0.0};
        tri_upper<1>(zr, Ls, lv, nc, eps, bad);
        if (lane < nc) zb[lane] = zr[0];
        if (blockIdx.x == 0) {
            if (lane < nc) z[tc + k0 + lane] = zr[0];
            flag_bad<1>(p, bad);
        }
    }
    __syncthreads();
    const int j = blockIdx.x * 64 + lane;
    const int kq = wv * 16, nq = min(16, nc - kq);
    double acc = 0.0;
    if (j < k0 && nq > 0) {
        const double* __restrict__ col = tv.S + (k0 + kq) + (size_t)j * nt;
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = col[min(q, nq - 1)];
#pragma unroll
        for (int q = 0; q < 16; q++)
            if (q < nq) acc += t[q] * zb[kq + q];
    }
    red[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && j < k0) z[tc + j] = z[tc + j] - (((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane]);
}

// ------------------------------------------- dense-tail sweeps, one launch
// Sync-free block-row chains: workgroup i owns 64-row block i of the tail
// and waits, block by block, for the blocks it depends on.  Each block's z
// is handed on as epoch-tagged granules (gran_put / gran_wait above,
// MI355X_MICROARCH.md hand-off table row R2: the data is the flag -- one
// store round trip on the producer, one load round trip on the consumer;
// round 2's sc1 payload + drained flag took two of each).  One workgroup
// per CU is enforced with dynamic LDS.  Every workgroup only waits on blocks
// of lower rank in its own launch order, so the grid drains as long as it
// is resident (ntb <= kChainMaxBlocks).
constexpr size_t kChainLds = 96 * 1024;
static_assert(2 * PC * (PC + 1) * sizeof(double) <= kChainLds, "k_tail_bwd_chain scratch");

#ifndef IPO_POLL_SLEEP
#define IPO_POLL_SLEEP 1
#endif
__device__ __forceinline__ void chain_wait(const int* flags, int j, int epoch) {
    if (threadIdx.x == 0)
        while (__hip_atomic_load(const_cast<int*>(flags + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch)
            __builtin_amdgcn_s_sleep(IPO_POLL_SLEEP);
    __syncthreads();
}

// Data-tagged hand-off of a block's z (MI355X_MICROARCH.md hand-off table,
// row R2): every double travels as two naturally aligned 8-byte granules
// {tag = epoch, 32-bit half}, each written by ONE relaxed agent-scope
// (sc1) store -- no flag, no drain, no barrier on the producer; the consumer
// re-reads its granules until every tag is the launch's epoch and has the
// data with the match.  Epochs grow by one per launch and are never reused
// (the buffer starts zeroed, the first epoch is 1), so no reset per launch.
// Block j, right-hand side r, row q: granules ((j R + r) 64 + q) 2 + {0, 1}.
typedef unsigned long long gran_t;
__device__ __forceinline__ void gran_put(gran_t* g, unsigned epoch, double v) {
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    const unsigned long long e = static_cast<unsigned long long>(epoch) << 32;
    __hip_atomic_store(g, e | (b & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, e | (b >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one wave: lane q < nr waits for row q of block j's R values
template <int R>
__device__ __forceinline__ void gran_wait(const gran_t* g, unsigned epoch, int lane, int nr, double (&v)[R]) {
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (lane < nr) {
                const gran_t* q = g + ((size_t)r * 64 + lane) * 2;
                const unsigned long long lo = __hip_atomic_load(const_cast<gran_t*>(q), __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long hi = __hip_atomic_load(const_cast<gran_t*>(q + 1), __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT);
                ok &= (lo >> 32) == epoch && (hi >> 32) == epoch;
                v[r] = __longlong_as_double(static_cast<long long>(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull)));
            } else {
                v[r] = 0.0;
            }
        }
        if (__all(ok)) return;
        __builtin_amdgcn_s_sleep(IPO_POLL_SLEEP);
    }
}

// forward: z_i -= sum_{j<i} L(i, j) z_j, then the unit-lower L11 solve of block i
template <int R>
__global__ void __launch_bounds__(NT)
k_tail_fwd_chain(PlanView p, TailView tv, SweepVecs V, const double* __restrict__ epsp, gran_t* __restrict__ gran,
                 unsigned epoch) {
    extern __shared__ double lds_pad[];
    __shared__ double Ls[PC][PC + 1];
    __shared__ int lv[PC];
    __shared__ double zb[R][PC];
    __shared__ double red[R][4][64];
    const int nt = tv.nt, tc = tv.tc, i = blockIdx.x, k0 = i * PC, nc = min(PC, nt - k0);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // the own block's right-hand side and eps do not depend on the chain
    double eps[R], zown[R];
    load_eps<R>(epsp, eps);
#pragma unroll
    for (int r = 0; r < R; r++) zown[r] = (wv == 0 && lane < nc) ? V.z[r * V.zs + tc + k0 + lane] : 0.0;
    if (tid == 0) lds_pad[0] = 0.0;
    stage_l11(tv.S + k0 + (size_t)k0 * nt, nt, nc, Ls);
    if (tid < nc) lv[tid] = p.live[tc + k0 + tid];
    const int row = k0 + (lane < nc ? lane : 0);
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    for (int j = 0; j < i; j++) {
        // the L(i, j) tile does not depend on z: load it before waiting
        const double* __restrict__ col = tv.S + row + (size_t)(j * PC + wv * 16) * nt;
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = col[(size_t)q * nt];
        if (wv == 0) {
            double zj[R];
            gran_wait<R>(gran + (size_t)j * R * 128, epoch, lane, PC, zj);
#pragma unroll
            for (int r = 0; r < R; r++) zb[r][lane] = zj[r];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) {
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] += t[q] * zb[r][wv * 16 + q];
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < R; r++) red[r][wv][lane] = acc[r];
    __syncthreads();
    if (wv == 0) {
        int bad[R] = {};
        double zr[R];
#pragma unroll
        for (int r = 0; r < R; r++)
            zr[r] = lane < nc ? zown[r] - (((red[r][0][lane] + red[r][1][lane]) + red[r][2][lane]) + red[r][3][lane])
                              : 0.0;
        tri_lower<R>(zr, Ls, lv, nc, eps, bad);
        if (lane < nc) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                gran_put(gran + (((size_t)i * R + r) * 64 + lane) * 2, epoch, zr[r]);
                V.z[r * V.zs + tc + k0 + lane] = zr[r];
            }
        }
        flag_bad<R>(p, bad);
    }
}

// backward (launch order = blocks from the last): z_i = D^{-1} z_i
// - sum_{j>i} L(j, i)' z_j, then the L11' solve.  Wave w owns 16 columns of
// block i, lanes stride the rows of block j (coalesced column reads).
template <int R>
__global__ void __launch_bounds__(NT)
k_tail_bwd_chain(PlanView p, TailView tv, SweepVecs V, const double* __restrict__ epsp, gran_t* __restrict__ gran,
                 unsigned epoch) {
    extern __shared__ double lds_pad[];
    __shared__ double Ls[PC][PC + 1];     // Ls[j][r] = L(j, r)
    __shared__ int lv[PC];
    __shared__ double zb[R][PC];
    __shared__ double xs[R][PC];
    const int nt = tv.nt, tc = tv.tc, ntb = tv.ntb;
    const int i = ntb - 1 - blockIdx.x, k0 = i * PC, nc = min(PC, nt - k0);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) lds_pad[0] = 0.0;
    stage_l11(tv.S + k0 + (size_t)k0 * nt, nt, nc, Ls);
    if (tid < nc) lv[tid] = p.live[tc + k0 + tid];
    const int kq = wv * 16, nq = min(16, nc - kq);
    // D^{-1} z of the own block does not depend on the chain: formed first,
    // by the wave that solves its right-hand side (wave r solves r: the two
    // triangular solves of R = 2 are independent chains, one wave each runs
    // them at about twice the pace of one wave interleaving both)
    double eps[R], zd[R];
    int bad[R] = {};
    load_eps<R>(epsp, eps);
#pragma unroll
    for (int r = 0; r < R; r++)
        zd[r] = (wv == r && lane < nc) ? dscale_rule(p, tc + k0 + lane, V.z[r * V.zs + tc + k0 + lane], eps[r], bad[r])
                                       : 0.0;
    double acc[R][16];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int q = 0; q < 16; q++) acc[r][q] = 0.0;
    for (int j = ntb - 1; j > i; j--) {
        const int r0 = j * PC, nr = min(PC, nt - r0);
        const int rr = r0 + (lane < nr ? lane : 0);
        const double* __restrict__ col = tv.S + rr + (size_t)(k0 + (nq > 0 ? kq : 0)) * nt;
        double t[16];
#pragma unroll
        for (int q = 0; q < 16; q++) t[q] = col[(size_t)min(q, max(nq, 1) - 1) * nt];
        if (wv == 0) {
            double zj[R];
            gran_wait<R>(gran + (size_t)j * R * 128, epoch, lane, nr, zj);
#pragma unroll
            for (int r = 0; r < R; r++) zb[r][lane] = zj[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double zr = lane < nr ? zb[r][lane] : 0.0;
#pragma unroll
            for (int q = 0; q < 16; q++) acc[r][q] += t[q] * zr;
        }
        __syncthreads();
    }
    double* red = lds_pad;   // colsum scratch
    if (nq > 0) colsum_put<R>(red, acc, kq, nq, lane);
    __syncthreads();
    if (tid < R * PC && tid % PC < nc) xs[tid / PC][tid % PC] = colsum_tree(red, tid / PC, tid % PC);
    __syncthreads();
    if (wv < R) {
        const int r = wv;
        double zr[1] = {lane < nc ? zd[r] - (i < ntb - 1 ? xs[r][lane] : 0.0) : 0.0};
        const double e1[1] = {eps[r]};
        int b1[1] = {bad[r]};
        tri_upper<1>(zr, Ls, lv, nc, e1, b1);
        if (lane < nc) {
            gran_put(gran + (((size_t)i * R + r) * 64 + lane) * 2, epoch, zr[0]);
            V.z[r * V.zs + tc + k0 + lane] = zr[0];
        }
        if (b1[0]) atomicOr(&p.incons[r], 1);
    }
}

// The backward chain with two 64-row blocks per workgroup ("pairs"): the
// first block's z is handed to the second inside the workgroup (through LDS
// after a barrier) instead of through memory, one hand-off per pair instead
// of per block, while the first block's z is published at once for the
// workgroups further down the chain.  Every entry sees the arithmetic of
// k_tail_bwd_chain in the same order (the partial sums over the earlier
// blocks, the internal block as their last term, the same column reductions
// and triangular solves): bitwise the same sweep.  From the last block:
// workgroup g owns blocks hi = ntb - 1 - 2g and lo = hi - 1 (none for an
// odd count's first workgroup).
constexpr size_t kPairBwdLds = 2 * PC * (PC + 1) * sizeof(double);           // colsum scratch (R <= 2)

template <int R>
__global__ void __launch_bounds__(NT)
k_tail_bwd_pair(PlanView p, TailView tv, SweepVecs V, const double* __restrict__ epsp, gran_t* __restrict__ gran,
                unsigned epoch) {
    extern __shared__ double lds_pad[];
    __shared__ double Ls[2][PC][PC + 1];     // [0] block hi, [1] block lo; Ls[j][r] = L(j, r)
    __shared__ int lv[2][PC];
    __shared__ double zb[R][PC];
    __shared__ double xs[R][PC];
    const int nt = tv.nt, tc = tv.tc, ntb = tv.ntb;
    const int hi = ntb - 1 - 2 * blockIdx.x, lo = hi - 1;
    const bool haslo = lo >= 0;
    const int kh = hi * PC, nch = min(PC, nt - kh), kl = haslo ? lo * PC : kh, ncl = haslo ? PC : 0;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    stage_l11(tv.S + kh + (size_t)kh * nt, nt, nch, Ls[0]);
    if (haslo) stage_l11(tv.S + kl + (size_t)kl * nt, nt, ncl, Ls[1]);
    if (tid < nch) lv[0][tid] = p.live[tc + kh + tid];
    if (tid < ncl) lv[1][tid] = p.live[tc + kl + tid];
    const int kq = wv * 16, nqh = min(16, nch - kq), nql = min(16, ncl - kq);
    double eps[R], zdh[R], zdl[R];
    int badh[R] = {}, badl[R] = {};
    load_eps<R>(epsp, eps);
#pragma unroll
    for (int r = 0; r < R; r++) {
        zdh[r] = (wv == 0 && lane < nch) ? dscale_rule(p, tc + kh + lane, V.z[r * V.zs + tc + kh + lane], eps[r], badh[r])
                                         : 0.0;
        zdl[r] = (wv == 0 && lane < ncl) ? dscale_rule(p, tc + kl + lane, V.z[r * V.zs + tc + kl + lane], eps[r], badl[r])
                                         : 0.0;
    }
    double acch[R][16], accl[R][16];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int q = 0; q < 16; q++) { acch[r][q] = 0.0; accl[r][q] = 0.0; }
    for (int j = ntb - 1; j > hi; j--) {
        const int r0 = j * PC, nr = min(PC, nt - r0);
        const int rr = r0 + (lane < nr ? lane : 0);
        const double* __restrict__ colh = tv.S + rr + (size_t)(kh + (nqh > 0 ? kq : 0)) * nt;
        const double* __restrict__ coll = tv.S + rr + (size_t)(kl + (nql > 0 ? kq : 0)) * nt;
        double th[16], tl[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
            th[q] = colh[(size_t)min(q, max(nqh, 1) - 1) * nt];
            tl[q] = coll[(size_t)min(q, max(nql, 1) - 1) * nt];
        }
        if (wv == 0) {
            double zj[R];
            gran_wait<R>(gran + (size_t)j * R * 128, epoch, lane, nr, zj);
#pragma unroll
            for (int r = 0; r < R; r++) zb[r][lane] = zj[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double zr = lane < nr ? zb[r][lane] : 0.0;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                acch[r][q] += th[q] * zr;
                accl[r][q] += tl[q] * zr;
            }
        }
        __syncthreads();
    }
    // block lo's term of block hi (rows of hi, columns of lo): loaded before hi's solve
    double tlh[16];
    {
        const int rr = kh + (lane < nch ? lane : 0);
        const double* __restrict__ col = tv.S + rr + (size_t)(kl + (nql > 0 ? kq : 0)) * nt;
#pragma unroll
        for (int q = 0; q < 16; q++) tlh[q] = col[(size_t)min(q, max(nql, 1) - 1) * nt];
    }
    double* red = lds_pad;   // colsum scratch
    if (hi < ntb - 1) {
        if (nqh > 0) colsum_put<R>(red, acch, kq, nqh, lane);
        __syncthreads();
        if (tid < R * PC && tid % PC < nch) xs[tid / PC][tid % PC] = colsum_tree(red, tid / PC, tid % PC);
        __syncthreads();
    }
    if (wv == 0) {
        double zr[R];
#pragma unroll
        for (int r = 0; r < R; r++) zr[r] = lane < nch ? zdh[r] - (hi < ntb - 1 ? xs[r][lane] : 0.0) : 0.0;
        tri_upper<R>(zr, Ls[0], lv[0], nch, eps, badh);
        if (lane < nch) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                gran_put(gran + (((size_t)hi * R + r) * 64 + lane) * 2, epoch, zr[r]);
                V.z[r * V.zs + tc + kh + lane] = zr[r];
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) zb[r][lane] = zr[r];
        flag_bad<R>(p, badh);
    }
    if (!haslo) return;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; r++) {
        const double zr = lane < nch ? zb[r][lane] : 0.0;
#pragma unroll
        for (int q = 0; q < 16; q++) accl[r][q] += tlh[q] * zr;
    }
    if (nql > 0) colsum_put<R>(red, accl, kq, nql, lane);
    __syncthreads();
    if (tid < R * PC && tid % PC < ncl) xs[tid / PC][tid % PC] = colsum_tree(red, tid / PC, tid % PC);
    __syncthreads();
    if (wv == 0) {
        double zr[R];
#pragma unroll
        for (int r = 0; r < R; r++) zr[r] = lane < ncl ? zdl[r] - xs[r][lane] : 0.0;
        tri_upper<R>(zr, Ls[1], lv[1], ncl, eps, badl);
        if (lane < ncl) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                gran_put(gran + (((size_t)lo * R + r) * 64 + lane) * 2, epoch, zr[r]);
                V.z[r * V.zs + tc + kl + lane] = zr[r];
            }
        }
        flag_bad<R>(p, badl);
    }
}

// ------------------------------------ forward tail sweep: a lead workgroup
// The chain above hands every block's z across CUs (a granule round trip per
// block on the critical path).  Here ONE lead workgroup solves all blocks in
// order, z_{i-1} reaching block i through LDS.  Of block i's products
// L(i, j) z_j the lead forms only the last K = kLeadBlocks (j = i-K .. i-1);
// helper workgroup i - K (one per block i > K) sums j = 0 .. i-K-1 from the
// granules of z the lead publishes and hands its per-lane partials to the
// lead as granules.  Each lane's sum is k_tail_fwd_chain's wave partial --
// the same terms in the same order, continued by the lead -- and the column
// reduction and L11 solve are the same: bitwise the same sweep.
// Lead: wave 0 solves; four "product waves" (column group g owns columns
// 16g .. 16g+15 of every block; waves 1, 2, 3, 5 -- wave 4, which would share
// the solver's SIMD, leaves at once) form the partials and, while wave 0
// solves block i, already sum block i+1's partial up to j = i-1, store the
// L11 of block i+1 (loaded a step earlier) and issue the loads of step i+2
// (tiles, L11, the helper partial).  Measured on dfl001 (70 blocks, R = 2,
// IPO_LEAD_STAMPS): 2.8 us per step -- solve 2.0, waits 0.8 -- against
// ~3.5 us per block of the per-block chain, whose cross-CU hand-off this
// removes.  Step i, barriers A_i and B_i:
//   products: acc = pre_i + L(i, i-1) z_{i-1} -> red  |A_i|  pre_{i+1} =
//             helper partial + L(i+1, j) z_j for j = i+1-K .. i-1; loads
//             for step i+2; L11(i+1) staged  |B_i|
//   solver:   |A_i|  z_i = L11 \ (z_i - sum of red), published  |B_i|
// Residency: a helper waits only on z the lead publishes, the lead only on
// helpers' partials over earlier z -- acyclic while the grid (<= ntb
// workgroups, one per CU by the dynamic LDS) is resident.
constexpr int kLeadBlocks = 2;     // K = 1 measured: forward sweep 380 -> 387 us (helpers' partials late)
// developer stamps (-DIPO_LEAD_STAMPS; compiled out otherwise): one launch's
// per-step split printed from the device
#ifdef IPO_LEAD_STAMPS
__device__ double g_lead_stats[8][4];
#define LEAD_T(v) const long long v = wall_clock64()
#else
#define LEAD_T(v) do {} while (0)
#endif
// raw buffer over the tail S (nt <= kChainMaxBlocks * PC: byte offsets fit an int)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tail_rsrc(const double* S) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(S), 0, 0x7fffffff, 0x00020000);
}
// (SC1: an sc1 load, which bypasses the CU's L1 -- the trailing form's reads
// of what k_tail_run stores meanwhile; aux bit 4 is sc1 on gfx942 / gfx950)
template <bool SC1 = false>
__device__ __forceinline__ double buf_ld(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    const i32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, SC1 ? 16 : 0);
    return __builtin_bit_cast(double, v);
}
constexpr int kLeadNT = 448;
constexpr int kHelpBatch = 4;
// helper partials: block i, right-hand side r, column group g, lane l ->
// granules ((((i R + r) 4 + g) 64 + l) 2 + {0, 1}
__device__ __forceinline__ gran_t* part_slot(gran_t* pg, int i, int R, int r, int g, int lane) {
    return pg + (((((size_t)i * R + r) * 4 + g) * 64) + lane) * 2;
}
__device__ __forceinline__ void lds_sync() {     // LDS-only barrier: global stores need not drain
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The trailing form (TRAIL; IPO_HIP_LEAD_TRAIL, kkt_device.h): the same
// sweep launched behind or beside the dense tail's factor k_tail_run instead
// of after its read-back.  It reads block column c of the tail (the tiles
// L(i, c), the L11' of block c, its live marks) only once the run's counter
// cdone[c] has reached lead_col_target(nt, c): every panel workgroup of step
// c adds itself there after its last store of the step (TailRun::cdone; sc1
// stores, every wave's vmcnt(0), a barrier, one agent-scope add), and every
// such read here is an sc1 load issued after the poll that saw the count
// (MI355X_MICROARCH.md's hand-off table, first row, as k_tail_run's own).
// The lead's product waves wait for column min(i + 2, ntb - 1) before step
// i's loads (columns 0 and 1 before the first), each helper product wave for
// the columns of its batch.  Arithmetic, order, granules, V.z and
// p.incons are the other form's: with every counter complete at the start
// (the launch behind the run) the sweep is that form's, bitwise.
// Helpers: the grid has 1 + H workgroups, H <= ntb - 1 - K; a helper that has
// published block i's partial draws the next ticket (ticket k >= 1 is block
// K + k) until the blocks are out, so a few workgroups, not ntb, sit beside
// the run.  The launch's ticket counter starts at zero (tbase = 0; the run's
// counter reset clears it), so a launch that aborts leaves nothing to
// account for.
// Termination.  Every wait of this form is one of
//   (a) a poll of cdone[c] (col_wait),
//   (b) a helper's wait for the lead's z granules (gran_wait_bail),
//   (c) the lead's wait for a helper's partial (the loop in step()),
// and each of them also reads the run's bail word p.flags[kFlagTailBlock] on
// every trip and gives up when it is non-zero.  k_tail_run ends short of
// completing a column only through a panel that bails, which raises the bail
// word before it posts (panel_w_body: the zero test of a first pass, and a DEP pass's
// contradicted speculation, kBailRestore, alike), or through items that
// skip themselves because they read the bail word set (run_wait, pre_wait): so
// either every counter completes or the bail word becomes and stays non-zero
// while this launch lives (the host clears it only after both streams are at
// rest).  With the counters complete, (b) and (c) are the other form's
// waits: ticket k's block is held by a running workgroup once tickets < k
// are drawn, a helper holding block b waits only for z_j, j < b - K, which
// the lead publishes without waiting for any block >= b, and the lead at
// step i only for the partial of block i + 1.  A wave that gives up sets the
// workgroup's abort word in LDS and goes on to the next barrier B; every
// wave reads the word after each B and returns there, so no wave is left at
// a barrier and no workgroup waits for a granule of one that left -- its
// own polls read the bail word too.  An aborted launch's z, granules and partials
// are incomplete; the factorisation it trailed has bailed, so its pre-pass
// is dropped and the normal pass rewrites them (a later epoch).
#ifndef IPO_TRAIL_SLEEP
#define IPO_TRAIL_SLEEP 16     // ~1024 clocks between polls: the run takes ~26 us per column
#endif
// one wave: until cdone[c] >= lead_col_target(nt, c) (seen: a value loaded
// earlier, to hide the first round trip); false: the run bailed meanwhile
__device__ __forceinline__ bool col_wait(const int* cdone, const int* bailp, int nt, int c, int seen) {
    const int need = lead_col_target(nt, c);
    int ok = 1;
    seen = __builtin_amdgcn_readfirstlane(seen);
    while (seen < need) {
        if (__builtin_amdgcn_readfirstlane(sc1_load_int(bailp)) != 0) {
            ok = 0;
            break;
        }
        __builtin_amdgcn_s_sleep(IPO_TRAIL_SLEEP);
        seen = __builtin_amdgcn_readfirstlane(sc1_load_int(cdone + c));
    }
    asm volatile("" ::: "memory");     // the column's loads stay behind the poll
    return ok != 0;
}
// gran_wait that gives up (false) when the run has bailed
template <int R>
__device__ __forceinline__ bool gran_wait_bail(const gran_t* g, unsigned epoch, int lane, int nr, double (&v)[R],
                                               const int* bailp) {
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (lane < nr) {
                const gran_t* q = g + ((size_t)r * 64 + lane) * 2;
                const unsigned long long lo = __hip_atomic_load(const_cast<gran_t*>(q), __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT);
                const unsigned long long hi = __hip_atomic_load(const_cast<gran_t*>(q + 1), __ATOMIC_RELAXED,
                                                                __HIP_MEMORY_SCOPE_AGENT);
                ok &= (lo >> 32) == epoch && (hi >> 32) == epoch;
                v[r] = __longlong_as_double(static_cast<long long>(((hi & 0xffffffffull) << 32) | (lo & 0xffffffffull)));
            } else {
                v[r] = 0.0;
            }
        }
        if (__all(ok)) return true;
        if (__builtin_amdgcn_readfirstlane(sc1_load_int(bailp)) != 0) return false;
        __builtin_amdgcn_s_sleep(IPO_POLL_SLEEP);
    }
}
// dynamic LDS of the trailing form: the lead's two L11 buffers, z history,
// reduction scratch and marks, then the abort word
constexpr size_t kLeadTrailLds =
    (2 * PC * (PC + 1) + kLeadBlocks * 2 * PC + 2 * 4 * 64) * sizeof(double) + 2 * PC * sizeof(int) + 64;

template <int R, bool TRAIL = false>
__global__ void __launch_bounds__(kLeadNT)
k_tail_fwd_lead(PlanView p, TailView tv, SweepVecs V, const double* __restrict__ epsp, gran_t* __restrict__ gran,
                gran_t* __restrict__ pgran, unsigned epoch, int* __restrict__ ticket, int tbase,
                const int* __restrict__ cdone) {
    extern __shared__ double lds[];
    constexpr int K = kLeadBlocks;
    const int nt = tv.nt, tc = tv.tc, ntb = tv.ntb;
    const int* bailp = p.flags + kFlagTailBlock;
    int* const abort_p = reinterpret_cast<int*>(lds + 2 * PC * (PC + 1) + K * 2 * PC + 2 * 4 * 64) + 2 * PC;
    // waves: 0 solves (right-hand side 0; 6, on SIMD 2, solves 1 when R = 2:
    // two independent chains at one wave each); 1, 2, 3 and 5 are column
    // groups 0-3; 4 (which would share wave 0's SIMD) leaves at once
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = wv <= 3 ? wv - 1 : wv - 2;     // wave-uniform (scalar buffer offsets)
    const int pl = g * 64 + lane;
    // roles by ticket, not by blockIdx: the workgroup that draws ticket 0 is
    // the lead, ticket t > 0 the helper of block t + K.  A helper waits only
    // on z the lead publishes and the lead only on partials of helpers with
    // lower tickets, each drawn by a workgroup that is running or done, so
    // the grid drains on any share of the CUs (co-tenant kernels, shards on
    // one device) without relying on dispatch order (ADVICE/VERDICT r04)
    __shared__ int role_sh;
    if (tid == 0) {
        role_sh = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - tbase;
        if constexpr (TRAIL) *abort_p = 0;
    }
    __syncthreads();
    int role = role_sh;
    if (wv == 4 || (wv == 6 && (R == 1 || role > 0))) return;
    // helper of block i = role + K (TRAIL: then of the blocks of further tickets)
    while (role > 0) {
        if (TRAIL && role + K >= ntb) return;
        const int i = role + K, k0 = i * PC, nc = min(PC, nt - k0), jend = i - K;
        double* zb = lds;        // zb[(b R + r) PC + c]
        const __amdgpu_buffer_rsrc_t rs = tail_rsrc(tv.S);
        const int nt8 = nt * 8, g16 = __builtin_amdgcn_readfirstlane(g * 16);
        const int voff = (k0 + (lane < nc ? lane : 0)) * 8;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0.0;
        for (int j0 = 0; j0 < jend; j0 += kHelpBatch) {
            double t[kHelpBatch][16];
            if (wv > 0) {
                if constexpr (TRAIL) {     // the batch's columns readable
                    bool go = true;
                    for (int b = 0; b < kHelpBatch && go; b++) {
                        const int c = min(j0 + b, jend - 1);
                        go = col_wait(cdone, bailp, nt, c, sc1_load_int(cdone + c));
                    }
                    if (!go && lane == 0) *abort_p = 1;
                }
#pragma unroll
                for (int b = 0; b < kHelpBatch; b++) {
                    const int s0 = (min(j0 + b, jend - 1) * PC + g16) * nt8;
#pragma unroll
                    for (int q = 0; q < 16; q++) t[b][q] = buf_ld<TRAIL>(rs, voff, s0 + q * nt8);
                }
            } else {
                bool gone = false;     // (TRAIL) the run bailed: no further wait
#pragma unroll
                for (int b = 0; b < kHelpBatch; b++) {
                    if (j0 + b < jend && !gone) {
                        double zj[R];
                        if constexpr (TRAIL) {
                            if (!gran_wait_bail<R>(gran + (size_t)(j0 + b) * R * 128, epoch, lane, PC, zj, bailp)) {
                                if (lane == 0) *abort_p = 1;
                                gone = true;
                            }
                        } else {
                            gran_wait<R>(gran + (size_t)(j0 + b) * R * 128, epoch, lane, PC, zj);
                        }
#pragma unroll
                        for (int r = 0; r < R; r++) zb[(b * R + r) * PC + lane] = zj[r];
                    }
                }
            }
            lds_sync();
            if (TRAIL && *abort_p) return;
            if (wv > 0) {
#pragma unroll
                for (int b = 0; b < kHelpBatch; b++) {
                    if (j0 + b < jend) {
#pragma unroll
                        for (int q = 0; q < 16; q++) {
#pragma unroll
                            for (int r = 0; r < R; r++) acc[r] += t[b][q] * zb[(b * R + r) * PC + g * 16 + q];
                        }
                    }
                }
            }
            lds_sync();
        }
        if (wv > 0) {
#pragma unroll
            for (int r = 0; r < R; r++) gran_put(part_slot(pgran, i, R, r, g, lane), epoch, acc[r]);
        }
        if constexpr (!TRAIL) return;
        // the next block, by ticket (every wave read role_sh before the
        // batch loop's barriers: jend >= 1)
        if (tid == 0) role_sh = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - tbase;
        lds_sync();
        role = role_sh;
    }
    double(*Ls)[PC][PC + 1] = reinterpret_cast<double(*)[PC][PC + 1]>(lds);     // two buffers
    double* zh = lds + 2 * PC * (PC + 1);     // z of the last K blocks: zh[((j % K) R + r) PC + c]
    double* red = zh + K * R * PC;            // red[(r 4 + g) 64 + lane]
    int* lv = reinterpret_cast<int*>(red + R * 4 * 64);    // lv[buf PC + c]
    if (wv == 0 || wv == 6) {
        // ---- solver wave(s): right-hand side rs
        const int rs = wv == 0 ? 0 : 1;
        double eps[1] = {epsp[rs]}, zown[1];
        int bad[1] = {};
        zown[0] = lane < min(PC, nt) ? V.z[rs * V.zs + tc + lane] : 0.0;
#ifdef IPO_LEAD_STAMPS
        long long sa = 0, st = 0, sb = 0;
#endif
        lds_sync();                                                      // B_{-1}
        if (TRAIL && *abort_p) return;
        for (int i = 0; i < ntb; i++) {
            LEAD_T(t0);
            const int k0 = i * PC, nc = min(PC, nt - k0);
            double znext;
            const int k1 = k0 + PC, nc1 = i + 1 < ntb ? min(PC, nt - k1) : 0;
            znext = lane < nc1 ? V.z[rs * V.zs + tc + k1 + lane] : 0.0;
            lds_sync();                                                  // A_i
            LEAD_T(t1);
            double zr[1];
            {
                const double* rd = red + rs * 4 * 64 + lane;
                zr[0] = lane < nc ? zown[0] - (((rd[0] + rd[64]) + rd[128]) + rd[192]) : 0.0;
            }
            tri_lower<1, true>(zr, Ls[i & 1], lv + (i & 1) * PC, nc, eps, bad);
            LEAD_T(t2);
            if (lane < nc) {
                gran_put(gran + (((size_t)i * R + rs) * 64 + lane) * 2, epoch, zr[0]);
                V.z[rs * V.zs + tc + k0 + lane] = zr[0];
            }
            zh[((i % K) * R + rs) * PC + lane] = lane < nc ? zr[0] : 0.0;
            zown[0] = znext;
            lds_sync();                                                  // B_i
            if (TRAIL && *abort_p) return;
#ifdef IPO_LEAD_STAMPS
            LEAD_T(t3);
            sa += t1 - t0; st += t2 - t1; sb += t3 - t2;
#endif
        }
#ifdef IPO_LEAD_STAMPS
        if (lane == 0 && wv == 0) {
            g_lead_stats[0][0] = sa * 0.01 / ntb; g_lead_stats[0][1] = st * 0.01 / ntb;
            g_lead_stats[0][2] = sb * 0.01 / ntb;
        }
#endif
        if (bad[0]) atomicOr(&p.incons[rs], 1);
        return;
    }
    // ---- product waves
    // buffer loads: the per-column offsets are scalars, only the row offset
    // is a per-lane register (64 global loads would each hold a 64-bit address)
    const __amdgpu_buffer_rsrc_t rs = tail_rsrc(tv.S);
    const int nt8 = nt * 8, g16 = __builtin_amdgcn_readfirstlane(g * 16);
    auto load_tiles = [&](int i, double(&t)[K][16]) {     // L(i, j), j = i-K .. i-1 (j >= 0)
        const int k0 = i * PC, nc = min(PC, nt - k0);
        const int voff = (k0 + (lane < nc ? lane : 0)) * 8;
#pragma unroll
        for (int b = 0; b < K; b++) {
            const int s0 = (max(i - K + b, 0) * PC + g16) * nt8;
#pragma unroll
            for (int q = 0; q < 16; q++) t[b][q] = buf_ld<TRAIL>(rs, voff, s0 + q * nt8);
        }
    };
    // L11 of block i (stage_l11's rows r = g + 4q of Ls[r][c] = L(r, c), c < r)
    // and its live marks, loaded into registers a step before they are stored
    auto l11_load = [&](int i, double(&t)[16], int& lvv) {
        const int k0 = i * PC, nc = min(PC, nt - k0);
        const int voff = (k0 + lane) * 8;
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = g + 4 * q;
            const bool ok = r < nc && lane < r;
            t[q] = buf_ld<TRAIL>(rs, ok ? voff : 0, min(k0 + r, nt - 1) * nt8);   // masked when stored
        }
        if constexpr (TRAIL) lvv = sc1_load_int(p.live + tc + k0 + min(pl, nc - 1));
        else lvv = p.live[tc + k0 + min(pl, nc - 1)];
    };
    auto l11_store = [&](int i, const double(&t)[16], int lvv) {
        const int nc = min(PC, nt - i * PC);
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int r = g + 4 * q;
            Ls[i & 1][r][lane] = r < nc && lane < r ? t[q] : 0.0;
        }
        if (pl < nc) lv[(i & 1) * PC + pl] = lvv;
    };
    unsigned long long praw[R][2];
    auto part_load = [&](int i) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const gran_t* q = part_slot(pgran, i, R, r, g, lane);
            praw[r][0] = __hip_atomic_load(const_cast<gran_t*>(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            praw[r][1] = __hip_atomic_load(const_cast<gran_t*>(q + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    double pre[R];
#pragma unroll
    for (int r = 0; r < R; r++) pre[r] = 0.0;
    double tA[K][16], tB[K][16], lA[16], lB[16];
    int vA, vB;
#ifdef IPO_LEAD_STAMPS
    long long pw = 0, p3 = 0, p4 = 0;
    int polls = 0;
#endif
    if constexpr (TRAIL) {          // columns 0 and 1 readable
        const int c1 = min(1, ntb - 1);
        const int s0 = sc1_load_int(cdone), s1 = sc1_load_int(cdone + c1);
        if (!(col_wait(cdone, bailp, nt, 0, s0) && col_wait(cdone, bailp, nt, c1, s1)) && lane == 0) *abort_p = 1;
    }
    l11_load(0, lA, vA);
    l11_store(0, lA, vA);
    load_tiles(min(1, ntb - 1), tB);
    l11_load(min(1, ntb - 1), lB, vB);
    part_load(min(1, ntb - 1));
    lds_sync();                                                          // B_{-1}
    if (TRAIL && *abort_p) return;
    // cur / lcur: step i's tiles (and the L11 slot to refill), nxt / lnxt: step i+1's
    auto step = [&](int i, double(&cur)[K][16], double(&nxt)[K][16], double(&lcur)[16], int& vcur,
                    double(&lnxt)[16], int& vnxt) {
        // TRAIL: column min(i + 2, ntb - 1)'s count, loaded a phase before it is tested
        int cseen = 0;
        if constexpr (TRAIL) cseen = sc1_load_int(cdone + min(i + 2, ntb - 1));
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = pre[r];
        if (i >= 1) {                                  // the last term: z_{i-1}
            const double* z = zh + ((i - 1) % K) * R * PC + g * 16;
#pragma unroll
            for (int q = 0; q < 16; q++) {
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] += cur[K - 1][q] * z[r * PC + q];
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) red[(r * 4 + g) * 64 + lane] = acc[r];
        lds_sync();                                                      // A_i
        LEAD_T(u0);
        if (i + 1 < ntb) {
            l11_store(i + 1, lnxt, vnxt);
            if (i + 1 > K) {                           // helper i+1-K's partial (j <= i-K)
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int r = 0; r < R; r++) ok &= (praw[r][0] >> 32) == epoch && (praw[r][1] >> 32) == epoch;
                    if (__all(ok)) break;
                    if constexpr (TRAIL) {             // its helper gave up: so does the lead
                        if (__builtin_amdgcn_readfirstlane(sc1_load_int(bailp)) != 0) {
                            if (lane == 0) *abort_p = 1;
                            break;
                        }
                    }
#ifdef IPO_LEAD_STAMPS
                    polls++;
#endif
                    __builtin_amdgcn_s_sleep(IPO_POLL_SLEEP);
                    part_load(i + 1);
                }
                LEAD_T(u1);
#ifdef IPO_LEAD_STAMPS
                pw += u1 - u0;
#endif
#pragma unroll
                for (int r = 0; r < R; r++)
                    pre[r] = __longlong_as_double(static_cast<long long>(((praw[r][1] & 0xffffffffull) << 32) |
                                                                         (praw[r][0] & 0xffffffffull)));
            } else {
#pragma unroll
                for (int r = 0; r < R; r++) pre[r] = 0.0;
            }
#pragma unroll
            for (int b = 0; b < K - 1; b++) {          // j = i+1-K .. i-1, in order
                const int j = i + 1 - K + b;
                if (j >= 0) {
                    const double* z = zh + (j % K) * R * PC + g * 16;
#pragma unroll
                    for (int q = 0; q < 16; q++) {
#pragma unroll
                        for (int r = 0; r < R; r++) pre[r] += nxt[b][q] * z[r * PC + q];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);     // z reads one tile at a time (registers)
            }
        }
        LEAD_T(u2);
        // step i+2's loads, unconditional (clamped in range: a conditional
        // load would keep the old registers live across the branch)
        const int i2 = min(i + 2, ntb - 1);
        if constexpr (TRAIL) {
            if (!col_wait(cdone, bailp, nt, i2, cseen) && lane == 0) *abort_p = 1;
        }
        load_tiles(i2, cur);
        l11_load(i2, lcur, vcur);
        part_load(i2);
        LEAD_T(u3);
#ifdef IPO_LEAD_STAMPS
        p3 += u2 - u0; p4 += u3 - u2;
#endif
        lds_sync();                                                      // B_i
        return !(TRAIL && *abort_p);
    };
    int i = 0;
    for (; i + 1 < ntb; i += 2) {      // two steps per trip, unconditionally (no register merges)
        if (!step(i, tA, tB, lA, vA, lB, vB)) return;
        if (!step(i + 1, tB, tA, lB, vB, lA, vA)) return;
    }
    if (i < ntb) step(i, tA, tB, lA, vA, lB, vB);
#ifdef IPO_LEAD_STAMPS
    if (lane == 0) {
        g_lead_stats[wv][0] = pw * 0.01 / ntb; g_lead_stats[wv][1] = polls;
        g_lead_stats[wv][2] = p3 * 0.01 / ntb; g_lead_stats[wv][3] = p4 * 0.01 / ntb;
    }
#endif
}

// ------------------------------------------- sync-free sweeps, top levels
// The narrow top of the elimination tree (levels >= h_.sf_level, a few
// supernodes each) in one persistent launch per direction instead of one or
// two launches per level.  One workgroup per CU (dynamic LDS).  Workgroups
// draw the work items in list order from a global ticket counter (one
// agent-scope atomic per item, drawn one item ahead), and an item only waits
// on items earlier in the list (descendants forward, ancestors backward).
// An item is therefore only ever held by a running workgroup, and every item
// it waits on was drawn earlier by a running workgroup: the grid drains
// whatever share of the CUs the launch gets (co-tenant kernels, several
// shards on one device).  The counter is never reset within a run: each
// launch draws exactly nitems + gridDim.x tickets (every workgroup stops at
// its first ticket past the list), so the host passes the launch's base.
// Items (build_sync_free_plan, kkt_schedule.cpp): (s, -1) a whole supernode,
// (s, c >= 0) solve chunk c (64 rows) of a supernode on a chunked level.
// Forward, every chunk item solves the diagonal part itself; backward, the
// chunk whose arrival comes last finishes the supernode.  The lists hold no
// other code: k_fwd_sf takes any code but -1 as a chunk index, and the
// (s, -2) finish item k_bwd_sf still has a branch for is never built.
// Hand-offs follow MI355X_MICROARCH.md
// (inter-workgroup visibility, table row 1): the producer writes the values
// with sc1 stores, waits vmcnt(0), joins a barrier, and one lane adds to
// the consumer's counter or stores a flag (agent scope); the consumer polls
// from one lane, joins a barrier and reads the values with sc1 loads.  Each
// handed-off value sits in 128-B lines of its own producer (padded ybuf
// slices, the zpad mirror, per-chunk partials), written once per sweep, so
// no consumer can have cached a line before its producer wrote it.  The
// arithmetic per supernode is that of the per-level kernels (bitwise).
constexpr int kSfIdx = static_cast<int>(kChainLds / sizeof(int));   // update-list indices staged per item

struct SfView {
    const int2* items;
    int nitems;
    int* cnt;           // per supernode: arrivals (forward: child y producers; backward: chunks)
    int* flag;          // per supernode: epoch of its completed diagonal part (fwd) / finish (bwd)
    const int* need;    // per supernode: forward arrivals per sweep
    const int* parent;  // per supernode: parent inside the range, else -1
    const int* zbase;   // per supernode: its padded z slice
    const int* zpi;     // per column: padded z position, -1 outside the range
    double* zpad;       // padded z slices of R right-hand sides
    size_t zps;
    int epoch;
    int* ticket;        // work-item counter (see above)
    int tbase;          // its value when this launch starts
};

// next work item of this workgroup: thread 0's ticket, through LDS
__device__ __forceinline__ int sf_draw(const SfView& sf) {
    return __hip_atomic_fetch_add(sf.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - sf.tbase;
}
// End of an item: the next ticket goes to LDS before the item's last
// barrier (no extra barrier), then the hand-off of MI355X_MICROARCH.md.
__device__ __forceinline__ void sf_next(int* tk, int nxt) {
    if (threadIdx.x == 0) *tk = nxt;
    __syncthreads();
}

__device__ __forceinline__ void sf_arrive_next(int* c, int* tk, int nxt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) *tk = nxt;
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sf_publish_next(int* flags, int i, int epoch, int* tk, int nxt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) *tk = nxt;
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flags + i, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


// Forward pre-pass of deep trees (build_sync_free_plan): z_c -= the sum of
// the update values column c of the narrow range receives from below the
// range, in list order, one thread per column (eight loads in flight).
template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_pre(int ncols, const int* __restrict__ col, const int* __restrict__ eptr, const int* __restrict__ eidx,
          SweepVecs V) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= ncols) return;
    const int c = col[j];
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    int e = eptr[j];
    const int e1 = eptr[j + 1];
    for (; e + 7 < e1; e += 8) {
        int ix[8];
#pragma unroll
        for (int u = 0; u < 8; u++) ix[u] = eidx[e + u];
#pragma unroll
        for (int r = 0; r < R; r++) {
            double yv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) yv[u] = V.y[r * V.ys + ix[u]];
#pragma unroll
            for (int u = 0; u < 8; u++) acc[r] += yv[u];
        }
    }
    for (; e < e1; e++) {
        const int i0 = eidx[e];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] += V.y[r * V.ys + i0];
    }
#pragma unroll
    for (int r = 0; r < R; r++) V.z[r * V.zs + c] -= acc[r];
}

template <int R>
__global__ void __launch_bounds__(NT)
k_fwd_sf(PlanView p, SfView sf, const int* __restrict__ yrow_ptr, const int* __restrict__ yrow_idx,
         const int* __restrict__ chunk_r0, SweepVecs V, const double* __restrict__ epsp) {
    extern __shared__ double lds_pad[];
    __shared__ double zl[R][PC];
    __shared__ double Ls[PC][PC + 1];
    __shared__ int lv[PC];
    __shared__ double red[R][4][64];
    __shared__ int sptr[PC + 1];
    double eps[R];
    load_eps<R>(epsp, eps);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __shared__ int tk[2];
    if (tid == 0) { lds_pad[0] = 0.0; tk[0] = sf_draw(sf); }
    __syncthreads();
    for (int par_ = 0;; par_ ^= 1) {
        const int it = tk[par_];
        if (it >= sf.nitems) break;
        // the next item's ticket is drawn once this item's wait is over (its
        // atomic then overlaps the item's work, not the wait) and stored at
        // the item's last barrier
        int nxt = 0;
        int* const slot = &tk[par_ ^ 1];
        SF_STAMP(it, 0);
        const int2 w = sf.items[it];
        const int s = w.x, code = w.y;
        const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
        const int hb = p.rowptr[s + 1] - p.rowptr[s], h = nc + hb;
        const int par = sf.parent[s];
        const double* panel = p.Lx + p.off[s];
        if (code == -1) {
            // the factor does not depend on the hand-off: L11, the marks and
            // (whole supernodes, hb <= 128 rows: one per thread) this
            // thread's row of L21 are loaded before the wait
            double lr[PC];
            const bool pre = code == -1 && hb <= NT && tid < hb;
            if (code == -1 && hb > 0) {
                const double* __restrict__ row = panel + nc + min(tid, hb - 1);
#pragma unroll
                for (int k = 0; k < PC; k++) lr[k] = row[(size_t)min(k, nc - 1) * h];
            }
            stage_l11(panel, h, nc, Ls);
            if (tid < nc) lv[tid] = p.live[c0 + tid];
            // the update-list indices do not depend on the hand-off either
            const int eb = yrow_ptr[c0], ne = yrow_ptr[c0 + nc] - eb;
            int* sidx = reinterpret_cast<int*>(lds_pad);
            const bool stg = ne <= kSfIdx;
            if (stg)
                for (int e = tid; e < ne; e += NT) sidx[e] = yrow_idx[eb + e];
            if (tid <= nc) sptr[tid] = yrow_ptr[c0 + tid];
            chain_wait(sf.cnt, s, sf.epoch * sf.need[s]);
            SF_STAMP(it, 1);
            if (tid == 0) nxt = sf_draw(sf);
            SF_NOTE(it, 6, ne);
            fwd_diag<R, true, true>(p, s, yrow_ptr, yrow_idx, V, eps, zl, Ls, lv, stg ? sidx : nullptr, it,
                                    stg ? sptr : nullptr);
            SF_STAMP(it, 2);
            if (code == -1) {       // y_s = L21 z_s, one row per thread (k_forward)
                if (pre) {
                    double acc[R];
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r] = 0.0;
#pragma unroll
                    for (int k = 0; k < PC; k++)
                        if (k < nc) {
#pragma unroll
                            for (int r = 0; r < R; r++) acc[r] += lr[k] * zl[r][k];
                        }
#pragma unroll
                    for (int r = 0; r < R; r++) sc1_store(V.y + r * V.ys + p.ybase[s] + tid, acc[r]);
                }
                for (int i = hb <= NT ? hb : tid; i < hb; i += NT) {
                    const double* __restrict__ row = panel + nc + i;
                    double acc[R];
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r] = 0.0;
#pragma unroll 8
                    for (int k = 0; k < nc; k++) {
                        const double l = row[(size_t)k * h];
#pragma unroll
                        for (int r = 0; r < R; r++) acc[r] += l * zl[r][k];
                    }
#pragma unroll
                    for (int r = 0; r < R; r++) sc1_store(V.y + r * V.ys + p.ybase[s] + i, acc[r]);
                }
                if (par >= 0) { SF_STAMP(it, 3); sf_arrive_next(sf.cnt + par, slot, nxt); SF_STAMP(it, 4); }
                else { SF_STAMP(it, 3); sf_next(slot, nxt); SF_STAMP(it, 4); }
            }
        } else {
            // one 64-row chunk of a chunked supernode: the diagonal part
            // (every chunk item of the supernode solves it, so the chain
            // has one hand-off per level, not two; z_s to the zpad mirror,
            // whence the backward sweep takes it), then y over the chunk's
            // rows (k_fwd_gemv)
            const int i = chunk_r0[code] + lane, kq = wv * 16, nq = min(16, nc - kq);
            double t[16];             // the factor tile, L11, the marks and the list indices before the wait
            {
                const double* __restrict__ row = panel + nc + min(i, hb - 1) + (size_t)(nq > 0 ? kq : 0) * h;
#pragma unroll
                for (int q = 0; q < 16; q++) t[q] = row[(size_t)min(q, max(nq, 1) - 1) * h];
            }
            stage_l11(panel, h, nc, Ls);
            if (tid < nc) lv[tid] = p.live[c0 + tid];
            const int eb = yrow_ptr[c0], ne = yrow_ptr[c0 + nc] - eb;
            int* sidx = reinterpret_cast<int*>(lds_pad);
            const bool stg = ne <= kSfIdx;
            if (stg)
                for (int e = tid; e < ne; e += NT) sidx[e] = yrow_idx[eb + e];
            if (tid <= nc) sptr[tid] = yrow_ptr[c0 + tid];
            chain_wait(sf.cnt, s, sf.epoch * sf.need[s]);
            SF_STAMP(it, 1);
            if (tid == 0) nxt = sf_draw(sf);
            fwd_diag<R, true, true>(p, s, yrow_ptr, yrow_idx, V, eps, zl, Ls, lv, stg ? sidx : nullptr, it,
                                    stg ? sptr : nullptr, sf.zpad + sf.zbase[s], sf.zps);
            SF_STAMP(it, 2);
            double acc[R];
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = 0.0;
            if (i < hb && nq > 0) {
#pragma unroll
                for (int q = 0; q < 16; q++)
                    if (q < nq) {
#pragma unroll
                        for (int r = 0; r < R; r++) acc[r] += t[q] * zl[r][kq + q];
                    }
            }
#pragma unroll
            for (int r = 0; r < R; r++) red[r][wv][lane] = acc[r];
            __syncthreads();
            if (wv == 0 && i < hb) {
#pragma unroll
                for (int r = 0; r < R; r++)
                    sc1_store(V.y + r * V.ys + p.ybase[s] + i,
                              ((red[r][0][lane] + red[r][1][lane]) + red[r][2][lane]) + red[r][3][lane]);
            }
            if (par >= 0) { SF_STAMP(it, 3); sf_arrive_next(sf.cnt + par, slot, nxt); SF_STAMP(it, 4); }
            else { SF_STAMP(it, 3); sf_next(slot, nxt); SF_STAMP(it, 4); }
        }
    }
}

// z of row ri for the backward sweep: the padded mirror inside the range
// (pi = sf.zpi[ri], looked up before the hand-off wait)
template <int R>
__device__ __forceinline__ void sf_zrow(const SfView& sf, const SweepVecs& V, int ri, int pi, double (&zi)[R]) {
#pragma unroll
    for (int r = 0; r < R; r++) zi[r] = pi >= 0 ? sc1_load(sf.zpad + r * sf.zps + pi) : V.z[r * V.zs + ri];
}

// Wave r of a backward item solves right-hand side r (the R chains are
// independent; one wave each): z_s = D^-1 z_s - sub (dscale_rule on the
// prefetched own z, d, mark; ldlt.c:473-480), then L11', z_s to z and to the
// zpad mirror.  sub = the four wave partials of xs summed in k_bwd_finish's
// order (chunked supernodes) or xs[r][0] (whole ones).
template <int R>
__device__ __forceinline__ void bwd_sf_solve(const PlanView& p, const SfView& sf, const SweepVecs& V, int s, int c0,
                                             int nc, bool chunked, double zo, int lvo, double dgo,
                                             const double (&eps)[R], const double (*Ls)[PC + 1], const int* lv,
                                             const double (*xs)[4][PC], int r) {
    const int lane = threadIdx.x & 63;
    const double e1[1] = {r == 0 ? eps[0] : eps[R - 1]};
    int bad[1] = {};
    double zr[1];
    {
        const double sub = chunked ? ((xs[r][0][lane] + xs[r][1][lane]) + xs[r][2][lane]) + xs[r][3][lane]
                                   : xs[r][0][lane];
        double zd = 0.0;
        if (lane < nc) {
            zd = zo;
            if (lvo) zd = zd / dgo;
            else if (fabs(zd) > e1[0]) bad[0] = 1;
            else zd = 0.0;
        }
        zr[0] = lane < nc ? zd - sub : 0.0;
    }
    tri_upper<1, true>(zr, Ls, lv, nc, e1, bad);
    if (lane < nc) {
        V.z[r * V.zs + c0 + lane] = zr[0];
        sc1_store(sf.zpad + r * sf.zps + sf.zbase[s] + lane, zr[0]);
    }
    if (bad[0]) atomicOr(&p.incons[r], 1);
}

template <int R>
__global__ void __launch_bounds__(NT)
k_bwd_sf(PlanView p, SfView sf, const int* __restrict__ chunk_r0, const int* __restrict__ sup_chunk0,
         double* __restrict__ part, size_t ps, SweepVecs V, const double* __restrict__ epsp) {
    extern __shared__ double lds_pad[];
    __shared__ double Ls[PC][PC + 1];     // Ls[j][r] = L(j, r)
    __shared__ int lv[PC];
    __shared__ double xs[R][4][PC];
    double eps[R];
    load_eps<R>(epsp, eps);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* red = lds_pad;   // colsum scratch
    __shared__ int tk[2];
    __shared__ int lastc;
    if (tid == 0) { lds_pad[0] = 0.0; tk[0] = sf_draw(sf); }
    __syncthreads();
    for (int par_ = 0;; par_ ^= 1) {
        const int it = tk[par_];
        if (it >= sf.nitems) break;
        int nxt = 0;                // next ticket: drawn after this item's wait, stored at its last barrier
        int* const slot = &tk[par_ ^ 1];
        const int2 w = sf.items[it];
        const int s = w.x, code = w.y;
        const int c0 = p.col0[s], nc = p.col0[s + 1] - c0;
        const int hb = p.rowptr[s + 1] - p.rowptr[s], h = nc + hb;
        const int par = sf.parent[s];
        const double* panel = p.Lx + p.off[s];
        const int* __restrict__ rows = p.rows + p.rowptr[s];
        const int kq = wv * 16, nq = min(16, nc - kq);
        if (code >= 0) {
            // partial sums of one 64-row chunk (k_bwd_partial); the chunk
            // whose arrival comes last finishes the supernode (k_bwd_finish:
            // the partials in its order, D^-1, L11') -- one hand-off per
            // level instead of a finish item waiting on the chunks
            const int i = chunk_r0[code] + lane;
            const bool okr = i < hb;
            const int ic = okr ? i : 0;
            const int ri = rows[ic];
            const int pi = sf.zpi[ri];
            double t[16];             // the factor tile, L11, the own z / d / mark before the wait
            const double* __restrict__ col = panel + nc + ic + (size_t)(nq > 0 ? kq : 0) * h;
#pragma unroll
            for (int q = 0; q < 16; q++) t[q] = col[(size_t)min(q, max(nq, 1) - 1) * h];
            stage_l11(panel, h, nc, Ls);
            if (tid < nc) lv[tid] = p.live[c0 + tid];
            double zown = 0.0, dgo = 1.0;     // of the right-hand side wave wv < R solves
            int lvo = 1;
            if (wv < R && lane < nc) {
                zown = sc1_load(sf.zpad + wv * sf.zps + sf.zbase[s] + lane);
                lvo = p.live[c0 + lane];
                dgo = p.dg[c0 + lane];
            }
            if (par >= 0) chain_wait(sf.flag, par, sf.epoch);
            if (tid == 0) nxt = sf_draw(sf);
            if (nq > 0) {
                double zi[R], v[R][16];
                sf_zrow<R>(sf, V, ri, pi, zi);
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int q = 0; q < 16; q++) v[r][q] = okr ? t[q] * zi[r] : 0.0;
                colsum_put<R>(red, v, kq, nq, lane);
            }
            __syncthreads();
            if (tid < R * PC && tid % PC < nc)
                sc1_store(part + (tid / PC) * ps + (size_t)code * PC + tid % PC, colsum_tree(red, tid / PC, tid % PC));
            const int nch = (hb + 63) / 64;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const int prev = __hip_atomic_fetch_add(sf.cnt + s, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                lastc = prev + 1 == sf.epoch * nch;
                *slot = nxt;
            }
            __syncthreads();
            if (!lastc) continue;
            const int cf = sup_chunk0[s];
            double x[R];
#pragma unroll
            for (int r = 0; r < R; r++) x[r] = 0.0;
            if (lane < nc)
                for (int c = wv; c < nch; c += 4) {
#pragma unroll
                    for (int r = 0; r < R; r++) x[r] += sc1_load(part + r * ps + (size_t)(cf + c) * PC + lane);
                }
#pragma unroll
            for (int r = 0; r < R; r++) xs[r][wv][lane] = x[r];
            __syncthreads();
            if (wv < R) bwd_sf_solve<R>(p, sf, V, s, c0, nc, true, zown, lvo, dgo, eps, Ls, lv, xs, wv);
            sf_publish_next(sf.flag, s, sf.epoch, slot, nxt);
            continue;
        }
        // nothing below depends on the hand-off but the z values of the
        // ancestors' rows and the chunk partials: L11, the marks, this
        // block's own z / d / mark (D^-1 z) and, for a whole supernode
        // (hb <= 128: two rows per lane at most), its L21 tiles and row
        // lookups are loaded before the wait
        stage_l11(panel, h, nc, Ls);
        if (tid < nc) lv[tid] = p.live[c0 + tid];
        double zown = 0.0, dgo = 1.0;     // of the right-hand side wave wv < R solves
        int lvo = 1;
        if (wv < R && lane < nc) {
            // a chunked supernode's forward z_s is in the zpad mirror (k_fwd_sf)
            zown = code == -2 ? sc1_load(sf.zpad + wv * sf.zps + sf.zbase[s] + lane) : V.z[wv * V.zs + c0 + lane];
            lvo = p.live[c0 + lane];
            dgo = p.dg[c0 + lane];
        }
        constexpr int kPre = 2;       // rows per lane prefetched (hb <= 128)
        double tp[kPre][16];
        int rip[kPre], pip[kPre];
        const bool pre = code == -1 && hb <= 64 * kPre && nq > 0;
        if (pre) {
#pragma unroll
            for (int u = 0; u < kPre; u++) {
                const int i = min(lane + 64 * u, max(hb - 1, 0));
                rip[u] = hb > 0 ? rows[i] : 0;
                const double* __restrict__ col = panel + nc + i + (size_t)kq * h;
#pragma unroll
                for (int q = 0; q < 16; q++) tp[u][q] = col[(size_t)min(q, nq - 1) * h];
            }
#pragma unroll
            for (int u = 0; u < kPre; u++) pip[u] = hb > 0 ? sf.zpi[rip[u]] : -1;
        }
        if (code == -2) chain_wait(sf.cnt, s, sf.epoch * ((hb + 63) / 64));
        else if (par >= 0) chain_wait(sf.flag, par, sf.epoch);
        if (tid == 0) nxt = sf_draw(sf);
        if (code == -2) {           // chunk partials in the order of k_bwd_finish
            const int cf = sup_chunk0[s], nch = (hb + 63) / 64;
            double x[R];
#pragma unroll
            for (int r = 0; r < R; r++) x[r] = 0.0;
            if (lane < nc)
                for (int c = wv; c < nch; c += 4) {
#pragma unroll
                    for (int r = 0; r < R; r++) x[r] += sc1_load(part + r * ps + (size_t)(cf + c) * PC + lane);
                }
#pragma unroll
            for (int r = 0; r < R; r++) xs[r][wv][lane] = x[r];
        } else if (pre) {           // L21' z_R from the prefetched tiles (same sums as below)
            double acc[R][16];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int q = 0; q < 16; q++) acc[r][q] = 0.0;
            double zi[kPre][R];
#pragma unroll
            for (int u = 0; u < kPre; u++)
                if (lane + 64 * u < hb) sf_zrow<R>(sf, V, rip[u], pip[u], zi[u]);
#pragma unroll
            for (int u = 0; u < kPre; u++)
                if (lane + 64 * u < hb) {
#pragma unroll
                    for (int q = 0; q < 16; q++)
                        if (q < nq) {
#pragma unroll
                            for (int r = 0; r < R; r++) acc[r][q] += tp[u][q] * zi[u][r];
                        }
                }
            colsum_put<R>(red, acc, kq, nq, lane);
        } else if (nq > 0) {        // L21' z_R over all rows (k_backward)
            double acc[R][16];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int q = 0; q < 16; q++) acc[r][q] = 0.0;
            for (int i = lane; i < hb; i += 64) {
                double zi[R];
                sf_zrow<R>(sf, V, rows[i], sf.zpi[rows[i]], zi);
                const double* __restrict__ col = panel + nc + i + (size_t)kq * h;
                double t[16];
#pragma unroll
                for (int q = 0; q < 16; q++) t[q] = col[(size_t)min(q, nq - 1) * h];
#pragma unroll
                for (int q = 0; q < 16; q++)
                    if (q < nq) {
#pragma unroll
                        for (int r = 0; r < R; r++) acc[r][q] += t[q] * zi[r];
                    }
            }
            colsum_put<R>(red, acc, kq, nq, lane);
        }
        __syncthreads();
        if (code != -2) {
            if (tid < R * PC && tid % PC < nc) xs[tid / PC][0][tid % PC] = colsum_tree(red, tid / PC, tid % PC);
            __syncthreads();
        }
        if (wv < R) bwd_sf_solve<R>(p, sf, V, s, c0, nc, code == -2, zown, lvo, dgo, eps, Ls, lv, xs, wv);
        sf_publish_next(sf.flag, s, sf.epoch, slot, nxt);
    }
}

__global__ void k_scale_scalar(double* e, int n, double f) { if (static_cast<int>(threadIdx.x) < n) e[threadIdx.x] *= f; }

}  // namespace

// The dynamic-LDS limit of the sweep kernels this plan launches (one
// workgroup per CU is enforced with dynamic LDS): sync_free, k_fwd_sf and
// k_bwd_sf of a plan with a sync-free range; else the dense tail's chain,
// pair and lead kernels (0 < ntb <= kChainMaxBlocks).
void KktDevice::raise_sweep_lds(bool sync_free) {
    struct Lds { const void* f; int bytes; };
    auto raise = [](std::initializer_list<Lds> table) {
        for (const Lds& e : table)
            IPO_HIP_CHECK(hipFuncSetAttribute(e.f, hipFuncAttributeMaxDynamicSharedMemorySize, e.bytes));
    };
    if (sync_free && h_.sf_level < plan_.nlevels)
        raise({{reinterpret_cast<const void*>(&k_fwd_sf<1>), kChainLds},
               {reinterpret_cast<const void*>(&k_fwd_sf<2>), kChainLds},
               {reinterpret_cast<const void*>(&k_bwd_sf<1>), kChainLds},
               {reinterpret_cast<const void*>(&k_bwd_sf<2>), kChainLds}});
    if (!sync_free && plan_.nt > 0 && plan_.ntb <= kChainMaxBlocks)
        raise({{reinterpret_cast<const void*>(&k_tail_fwd_chain<1>), kChainLds},
               {reinterpret_cast<const void*>(&k_tail_fwd_chain<2>), kChainLds},
               {reinterpret_cast<const void*>(&k_tail_bwd_chain<1>), kChainLds},
               {reinterpret_cast<const void*>(&k_tail_bwd_chain<2>), kChainLds},
               {reinterpret_cast<const void*>(&k_tail_bwd_pair<1>), kPairBwdLds},
               {reinterpret_cast<const void*>(&k_tail_bwd_pair<2>), kPairBwdLds},
               {reinterpret_cast<const void*>(&k_tail_fwd_lead<1>), kChainLds},
               {reinterpret_cast<const void*>(&k_tail_fwd_lead<2>), kChainLds},
               {reinterpret_cast<const void*>(&k_tail_fwd_lead<1, true>), static_cast<int>(kLeadTrailLds)},
               {reinterpret_cast<const void*>(&k_tail_fwd_lead<2, true>), static_cast<int>(kLeadTrailLds)}});
}

// Per-level summary of the last forward sync-free sweep's stamps (10 ns
// ticks): items, mean wait / diag (gather + L11 solve) / rest / hand-off,
// and when the level's last item finished.  Developer build with
// -DIPO_SF_STAMPS only (g_sfst above); called by ~KktDevice.
void KktDevice::dump_sf_stamps() const {
#ifdef IPO_SF_STAMPS
    const std::vector<SchedInt2>& items = h_sf_items_f_;
    const KktPlan& P = plan_;
    const std::string& file = knobs_.sf_stamps_file;
    if (items.empty()) return;
    std::vector<long long> st((size_t)(1 << 15) * 10);
    if (hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(g_sfst), st.size() * sizeof(long long)) != hipSuccess) return;
    const int n = std::min<int>(items.size(), 1 << 15);
    long long t0 = LLONG_MAX;
    for (int i = 0; i < n; i++) t0 = std::min(t0, st[i * 10]);
    std::map<int, std::array<double, 7>> lv;   // level -> items, wait, diag, rest, end, handoff, ...
    for (int i = 0; i < n; i++) {
        const long long* x = &st[i * 10];
        auto& a = lv[P.level[items[i].x]];
        a[0] += 1; a[1] += x[1] - x[0]; a[2] += x[2] - x[1]; a[3] += x[3] - x[2]; a[4] = std::max<double>(a[4], x[4] - t0);
        a[5] += x[4] - x[3];
    }
    if (!file.empty()) {
        if (FILE* fo = std::fopen(file.c_str(), "w")) {
            for (int i = 0; i < n; i++) {
                const long long* x = &st[i * 10];
                std::fprintf(fo, "%d %d %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", items[i].x, items[i].y,
                             P.level[items[i].x], P.parent[items[i].x], x[0] - t0, x[1] - t0, x[2] - t0, x[3] - t0,
                             x[4] - t0, x[5] - t0, x[6], x[7] - t0, x[8] - t0);
            }
            std::fclose(fo);
        }
    }
    std::fprintf(stderr, "sf forward: level items wait diag rest handoff end(us)\n");
    for (auto& [l, a] : lv)
        std::fprintf(stderr, "  %3d %4.0f %7.2f %7.2f %7.2f %6.2f %8.1f\n", l, a[0], a[1] / a[0] / 100, a[2] / a[0] / 100,
                     a[3] / a[0] / 100, a[5] / a[0] / 100, a[4] / 100);
#endif
}

// Substitution sweeps for R right-hand sides stored at dz + r * K: the two
// step lists of the schedule (h_.sweep, kkt_schedule.h), walked in order.
template <int R>
void KktDevice::sweep(double* dz, const double* epsp, size_t fwd_first) {
    hipStream_t s = stream_;
    if (timing_) IPO_HIP_CHECK(hipEventRecord(ev2_, s));
    ph_begin(s);
    const int nf = run_sweep_steps<R>(h_.sweep.fwd, true, dz, epsp, fwd_first);
    ph_end(kPhForward, nf, s);
    ph_begin(s);
    const int nb = run_sweep_steps<R>(h_.sweep.bwd, false, dz, epsp);
    ph_end(kPhBackward, nb, s);
    IPO_HIP_CHECK(hipGetLastError());
    if (timing_) {
        IPO_HIP_CHECK(hipEventRecord(ev3_, s));
        IPO_HIP_CHECK(hipEventSynchronize(ev3_));
        float ms = 0;
        IPO_HIP_CHECK(hipEventElapsedTime(&ms, ev2_, ev3_));
        tm_.sweep_ms += ms;
        ph_collect();
        tm_.phase_count[kPhForward]++;
        tm_.phase_count[kPhBackward]++;
    }
}

// One list of a sweep: every step launches its forward or its backward
// kernel(s) over the range it carries (SweepKind, kkt_schedule.h) and does the
// host bookkeeping that goes with that launch.  Returns the kernels launched,
// counted here and not taken from the schedule.  The TailBlock and TailDscale
// kernels take one right-hand side: a blocked tail's lists run with R = 1.
// The cases stand in SweepKind's order, which is also the order the compiler
// emits the kernel instances in; k_fwd_level<1> and k_fwd_leaf<1> get their
// address arithmetic scheduled differently unless k_forward<1> is emitted
// before them, so Plain stays ahead of the leaf kinds (device code compared
// across changes stays identical).  Steps [first, last) of the list (last
// clipped to its end), on stream s (null: the object's): the forward
// pre-pass runs the head of the forward list on the caller's side stream, and
// the solve that uses it the rest (kkt_device.h PrePass).
template <int R>
int KktDevice::run_sweep_steps(const std::vector<SweepStep>& steps, bool forward, double* dz, const double* epsp,
                               size_t first, size_t last, hipStream_t s) {
    if (!s) s = stream_;
    const PlanView pv = plan_view();
    const TailView tv = tail_view();
    const SweepVecs V{dz, static_cast<size_t>(T_), dYbuf_.get(), h_.ybuf_stride};
    const size_t ps = h_.partial_stride;
    const int nt = plan_.nt;
    int launched = 0;
    for (size_t i = first; i < std::min(last, steps.size()); i++) {
        const SweepStep& step = steps[i];
        const int q0 = step.q0, n = step.n;
        switch (step.kind) {
        case kSwChunked: {
            const int cb = step.a, nch = step.b;
            if (forward) {
                hipLaunchKernelGGL(k_fwd_diag<R>, dim3(n), dim3(NT), 0, s, pv, dsweep_sups_.get(), q0, dyrow_ptr_.get(),
                                   dyrow_idx_.get(), V, epsp);
                hipLaunchKernelGGL(k_fwd_gemv<R>, dim3(nch), dim3(NT), 0, s, pv, dchunk_sup_.get(), dchunk_r0_.get(),
                                   cb, V);
            } else {
                hipLaunchKernelGGL(k_bwd_partial<R>, dim3(nch), dim3(NT), 0, s, pv, dchunk_sup_.get(), dchunk_r0_.get(),
                                   cb, V, dPartial_.get(), ps);
                hipLaunchKernelGGL(k_bwd_finish<R>, dim3(n), dim3(NT), 0, s, pv, dsweep_sups_.get(), q0,
                                   dsup_chunk0_.get(), dPartial_.get(), ps, V, epsp);
            }
            launched++;      // two kernels
            break;
        }
        case kSwPlain:
            if (forward)
                hipLaunchKernelGGL(k_forward<R>, dim3(n), dim3(NT), 0, s, pv, dsweep_sups_.get(), q0, dyrow_ptr_.get(),
                                   dyrow_idx_.get(), V, epsp);
            else
                hipLaunchKernelGGL(k_backward<R>, dim3(n), dim3(NT), 0, s, pv, dsweep_sups_.get(), q0, V, epsp);
            break;
        case kSwLeaf8:
            if (forward)
                hipLaunchKernelGGL(k_fwd_leaf8<R>, dim3(ceil_div(n, NT / kSmallLeaf)), dim3(NT), 0, s, pv,
                                   dsweep_sups_.get(), q0, n, dyrow_ptr_.get(), dyrow_idx_.get(), V, epsp);
            else
                hipLaunchKernelGGL(k_bwd_leaf8<R>, dim3(ceil_div(n, NT / kSmallLeaf)), dim3(NT), 0, s, pv,
                                   dsweep_sups_.get(), q0, n, V, epsp);
            break;
        case kSwMerged: {
            const int nlb = ceil_div(n, NT / 64);
            if (forward)
                hipLaunchKernelGGL(k_fwd_level<R>, dim3(nlb + step.a), dim3(NT), 0, s, pv, dsweep_sups_.get(), q0, n,
                                   nlb, dyrow_ptr_.get(), dyrow_idx_.get(), V, epsp);
            else
                hipLaunchKernelGGL(k_bwd_level<R>, dim3(nlb + step.a), dim3(NT), 0, s, pv, dsweep_sups_.get(), q0, n,
                                   nlb, V, epsp);
            break;
        }
        case kSwLeaf:
            if (forward)
                hipLaunchKernelGGL(k_fwd_leaf<R>, dim3(ceil_div(n, NT / 64)), dim3(NT), 0, s, pv, dsweep_sups_.get(),
                                   q0, n, dyrow_ptr_.get(), dyrow_idx_.get(), V, epsp);
            else
                hipLaunchKernelGGL(k_bwd_leaf<R>, dim3(ceil_div(n, NT / 64)), dim3(NT), 0, s, pv, dsweep_sups_.get(),
                                   q0, n, V, epsp);
            break;
        case kSwPre:
            hipLaunchKernelGGL(k_fwd_pre<R>, dim3(ceil_div(n, NT)), dim3(NT), 0, s, n, dpre_col_.get(), dpre_ptr_.get(),
                               dpre_idx_.get(), V);
            break;
        case kSwSyncFree:      // the narrow top levels in one launch
            if (forward) {
                const SfView sf{dsf_items_f_.get(), n, dsf_fcnt_.get(), dsf_fflag_.get(), dsf_need_.get(),
                                dsf_par_.get(), dsf_zbase_.get(), dsf_zpi_.get(), dZpad_.get(), h_.zpad_stride,
                                ++sf_fwd_epoch_, dsf_ticket_.get(), sf_tbase(0, n, s)};
                const bool pre = step.a != 0;
                hipLaunchKernelGGL(k_fwd_sf<R>, dim3(std::min(sf_grid_, n)), dim3(NT), kChainLds, s, pv, sf,
                                   pre ? dylate_ptr_.get() : dyrow_ptr_.get(),
                                   pre ? dylate_idx_.get() : dyrow_idx_.get(), dchunk_r0_.get(), V, epsp);
            } else {
                const SfView sf{dsf_items_b_.get(), n, dsf_bcnt_.get(), dsf_bflag_.get(), dsf_need_.get(),
                                dsf_par_.get(), dsf_zbase_.get(), dsf_zpi_.get(), dZpad_.get(), h_.zpad_stride,
                                ++sf_bwd_epoch_, dsf_ticket_.get() + 1, sf_tbase(1, n, s)};
                hipLaunchKernelGGL(k_bwd_sf<R>, dim3(std::min(sf_grid_, n)), dim3(NT), kChainLds, s, pv, sf,
                                   dchunk_r0_.get(), dsup_chunk0_.get(), dPartial_.get(), ps, V, epsp);
            }
            break;
        case kSwTailGather:
            tail_rhs_begin(dz, R);
            hipLaunchKernelGGL(k_tail_gather<R>, dim3(ceil_div(nt, 4)), dim3(NT), 0, s, tv, dyrow_ptr_.get(),
                               dyrow_idx_.get(), V);
            tail_rhs_end(dz, R);
            break;
        case kSwTailLead: {
            const int grid = 1 + std::max(0, plan_.ntb - 1 - kLeadBlocks);
            if (lead_ticket_next_ + grid > (1LL << 30)) {
                IPO_HIP_CHECK(hipMemsetAsync(dlead_ticket_.get(), 0, sizeof(int), s));
                lead_ticket_next_ = 0;
            }
            const int tb = static_cast<int>(lead_ticket_next_);
            lead_ticket_next_ += grid;
            hipLaunchKernelGGL(k_tail_fwd_lead<R>, dim3(grid), dim3(kLeadNT), kChainLds, s, pv, tv, V, epsp,
                               dChainGran_.get(), dChainGran_.get() + ChainGran::part_at(plan_.ntb),
                               ++chain_epoch_, dlead_ticket_.get(), tb, static_cast<const int*>(nullptr));
#ifdef IPO_LEAD_STAMPS
            if (chain_epoch_ % 64 == 41) {
                double st[8][4];
                IPO_HIP_CHECK(hipStreamSynchronize(s));
                IPO_HIP_CHECK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_lead_stats), sizeof(st)));
                std::fprintf(stderr, "lead R %d ntb %d per step us: solver wait-A %.3f tri %.3f wait-B %.3f\n", R,
                             plan_.ntb, st[0][0], st[0][1], st[0][2]);
                for (int w = 1; w <= 4; w++)
                    std::fprintf(stderr, "  wave %d: partial wait %.3f (%g polls) phase3 %.3f loads %.3f\n", w,
                                 st[w][0], st[w][1], st[w][2], st[w][3]);
            }
#endif
            break;
        }
        case kSwTailChain:
            if (forward)
                hipLaunchKernelGGL(k_tail_fwd_chain<R>, dim3(plan_.ntb), dim3(NT), kChainLds, s, pv, tv, V, epsp,
                                   dChainGran_.get(), ++chain_epoch_);
            else
                hipLaunchKernelGGL(k_tail_bwd_chain<R>, dim3(plan_.ntb), dim3(NT), kChainLds, s, pv, tv, V, epsp,
                                   dChainGran_.get(), ++chain_epoch_);
            break;
        case kSwTailPair:
            hipLaunchKernelGGL(k_tail_bwd_pair<R>, dim3((plan_.ntb + 1) / 2), dim3(NT), kPairBwdLds, s, pv, tv, V, epsp,
                               dChainGran_.get(), ++chain_epoch_);
            break;
        case kSwTailBlock: {
            const int kb = step.a;
            if (forward) {
                const int below = nt - std::min(nt, (kb + 1) * kPanelCols);
                hipLaunchKernelGGL(k_tail_fwd, dim3(std::max(1, ceil_div(below, 64))), dim3(NT), 0, s, pv, tv, kb, dz,
                                   epsp);
            } else {
                const int left = kb * kPanelCols;
                hipLaunchKernelGGL(k_tail_bwd, dim3(std::max(1, ceil_div(left, 64))), dim3(NT), 0, s, pv, tv, kb, dz,
                                   epsp);
            }
            break;
        }
        case kSwTailDscale:
            hipLaunchKernelGGL(k_tail_dscale, dim3(ceil_div(nt, NT)), dim3(NT), 0, s, pv, tv, dz, epsp);
            break;
        default:
            throw std::logic_error("sweep: unknown step kind");
        }
        launched++;
    }
    return launched;
}

// The forward pre-pass's share of the forward list (kkt_device.h PrePass):
// steps [0, split) for the R right-hand sides in dZ_, on q.
void KktDevice::run_prepass_steps(int R, hipStream_t q) {
    double* epsp = sweep_eps();
    const size_t split = static_cast<size_t>(h_.sweep.split);
    if (R == 2) run_sweep_steps<2>(h_.sweep.fwd, true, dZ_.get(), epsp, 0, split, q);
    else run_sweep_steps<1>(h_.sweep.fwd, true, dZ_.get(), epsp, 0, split, q);
}

// The forward tail lead in its trailing form (k_tail_fwd_lead<R, true>;
// IPO_HIP_LEAD_TRAIL, kkt_device.h) for the pre-pass's R right-hand sides in
// dZ_, on s: behind k_tail_run on its own stream, with one helper per block
// as the other form, or beside it on the pre-pass's stream, with at most
// knobs_.lead_helpers helper workgroups that take the blocks by ticket, so
// that few CUs hold a poller's LDS while the run's visits want them.  Its
// ticket is RunCounters::lead_ticket (zeroed with the run's counters).
void KktDevice::launch_lead_trail(int R, hipStream_t s, bool beside) {
    const PlanView pv = plan_view();
    const TailView tv = tail_view();
    const SweepVecs V{dZ_.get(), static_cast<size_t>(T_), dYbuf_.get(), h_.ybuf_stride};
    const int nhb = std::max(0, plan_.ntb - 1 - kLeadBlocks);
    const int grid = 1 + (beside ? std::min(nhb, knobs_.lead_helpers) : nhb);
    const double* epsp = sweep_eps();
    gran_t* gran = dChainGran_.get();
    gran_t* pgran = gran + ChainGran::part_at(plan_.ntb);
    const RunCounters cnt = run_counters();
    if (R == 2)
        hipLaunchKernelGGL((k_tail_fwd_lead<2, true>), dim3(grid), dim3(kLeadNT), kLeadTrailLds, s, pv, tv, V, epsp, gran,
                           pgran, ++chain_epoch_, cnt.lead_ticket, 0, static_cast<const int*>(cnt.cdone));
    else
        hipLaunchKernelGGL((k_tail_fwd_lead<1, true>), dim3(grid), dim3(kLeadNT), kLeadTrailLds, s, pv, tv, V, epsp, gran,
                           pgran, ++chain_epoch_, cnt.lead_ticket, 0, static_cast<const int*>(cnt.cdone));
}

// Ticket base of the next sync-free launch of direction d over nitems items:
// each launch draws nitems + grid tickets; the counter is cleared (in stream
// order) before it could overflow.
int KktDevice::sf_tbase(int d, int nitems, hipStream_t s) {
    const long long draw = static_cast<long long>(nitems) + std::min(sf_grid_, nitems);
    if (sf_ticket_next_[d] + draw > (1LL << 30)) {
        IPO_HIP_CHECK(hipMemsetAsync(dsf_ticket_.get() + d, 0, sizeof(int), s));
        sf_ticket_next_[d] = 0;
    }
    const int base = static_cast<int>(sf_ticket_next_[d]);
    sf_ticket_next_[d] += draw;
    return base;
}

// Sharded sweeps: the tail rows' right-hand side enters once (shard 0), and
// after the gather each shard holds its own blocks' contributions: sum them.
void KktDevice::tail_rhs_begin(double* dz, int R) {
    if (!shard_minor()) return;
    for (int r = 0; r < R; r++)
        IPO_HIP_CHECK(hipMemsetAsync(dz + (size_t)r * T_ + plan_.tail_c0, 0, sizeof(double) * plan_.nt, stream_));
}
void KktDevice::tail_rhs_end(double* dz, int R) {
    for (int r = 0; r < R; r++) xsum(dz + (size_t)r * T_ + plan_.tail_c0, plan_.nt, RedOp::Sum);
}

// rawsolve (ldlt.c:433-505) of R right-hand sides at dz + r * K, in place.
void KktDevice::rawsolve(double* dz, int R, size_t fwd_first) {
    hipStream_t s = stream_;
    double* epsp = sweep_eps();             // eps of right-hand side r at epsp[r]
    if (ndep_ > 0) {
        // eps = epssol * max|z[0..n)| (ldlt.c:446: first n entries of the permuted vector)
        RedJobs j{};
        j.nj = R;
        for (int r = 0; r < R; r++) { j.a[r] = dz + (size_t)r * T_; j.b[r] = nullptr; j.len[r] = n_; j.op[r] = 1; }
        launch_reduce(j, dPart_.get(), epsp, s);
        hipLaunchKernelGGL(k_scale_scalar, dim3(1), dim3(64), 0, s, epsp, R, 1.0e-6);
        xsum(epsp, R, RedOp::Max);
    } else if (!eps_cleared_) {
        IPO_HIP_CHECK(hipMemsetAsync(epsp, 0, R * sizeof(double), s));
    }
    if (R == 2 && !h_.paths.tail_blocked) {
        sweep<2>(dz, epsp, fwd_first);
    } else {                         // (a blocked tail's per-block kernels: one right-hand side at a time)
        for (int r = 0; r < R; r++) sweep<1>(dz + (size_t)r * T_, epsp + r, fwd_first);
    }
    tm_.rawsolves += R;
}

}  // namespace ipo
