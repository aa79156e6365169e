// value_refresh.hip -- the device side of ipo_hip_ctx_update and of the start
// point entries (value_maps.h): gathers through the index maps, the
// validation reductions that run before anything is committed, and the
// clamped copy of ipo_hip_ctx_start_from_last.  All are grid-stride over a
// fixed grid; none is on a solve's path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "hip_util.h"
#include "value_maps.h"

namespace ipo {

namespace {

constexpr int kVT = 256;          // threads a block
constexpr int kVBlocksMax = 1024; // blocks at most (4 a CU on 256 CUs)

int grid_for(long items) { return static_cast<int>(std::max(1l, std::min<long>(kVBlocksMax, (items + kVT - 1) / kVT))); }

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ double gather1(const double* __restrict__ src, int k) { return k >= 0 ? src[k] : 0.0; }

// WIDE: four entries a step, the map as one int4 and dst as two double2 (the
// caller has checked both for 16-byte alignment); the n % 4 tail one by one
template <bool WIDE>
__global__ void __launch_bounds__(kVT)
k_gather_map(int n, const int* __restrict__ map, const double* __restrict__ src, double* __restrict__ dst) {
    const long stride = static_cast<long>(gridDim.x) * kVT;
    const long t = static_cast<long>(blockIdx.x) * kVT + threadIdx.x;
    if (WIDE) {
        const int n4 = n >> 2;
        for (long g = t; g < n4; g += stride) {
            const int4 k = reinterpret_cast<const int4*>(map)[g];
            double2 lo, hi;
            lo.x = gather1(src, k.x); lo.y = gather1(src, k.y);
            hi.x = gather1(src, k.z); hi.y = gather1(src, k.w);
            reinterpret_cast<double2*>(dst)[2 * g] = lo;
            reinterpret_cast<double2*>(dst)[2 * g + 1] = hi;
        }
        for (long i = (static_cast<long>(n4) << 2) + t; i < n; i += stride) dst[i] = gather1(src, map[i]);
    } else {
        for (long i = t; i < n; i += stride) dst[i] = gather1(src, map[i]);
    }
}

// the smallest index a thread found (INT_MAX: none) lowered into *first: the
// wave's minimum by shuffles, one atomicMin a wave that found any
__device__ __forceinline__ void publish_first(int mine, int* first) {
    for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_down(mine, o, 64));
    if ((threadIdx.x & 63) == 0 && mine != INT_MAX) atomicMin(first, mine);
}

__device__ __forceinline__ bool finite_bits(double v) {
    // exponent field all ones: NaN or Inf (no fast-math assumption to lose it)
    return ((__double_as_longlong(v) >> 52) & 0x7ff) != 0x7ff;
}

// KIND 0: not finite; 1: not finite or not > 0.  Two entries a load (16 bytes)
// when v is aligned (WIDE), entries taken in index order within a thread.
template <int KIND, bool WIDE>
__global__ void __launch_bounds__(kVT)
k_first_bad(int n, const double* __restrict__ v, int* __restrict__ first) {
    const long stride = static_cast<long>(gridDim.x) * kVT;
    const long t = static_cast<long>(blockIdx.x) * kVT + threadIdx.x;
    int mine = INT_MAX;
    auto bad = [](double a) { return !finite_bits(a) || (KIND == 1 && !(a > 0.0)); };
    if (WIDE) {
        const int n2 = n >> 1;
        for (long g = t; g < n2; g += stride) {
            const double2 a = reinterpret_cast<const double2*>(v)[g];
            const int i = static_cast<int>(g << 1);
            if (bad(a.y)) mine = min(mine, i + 1);
            if (bad(a.x)) mine = min(mine, i);
        }
        if ((n & 1) && t == 0 && bad(v[n - 1])) mine = min(mine, n - 1);
    } else {
        for (long i = t; i < n; i += stride)
            if (bad(v[i])) mine = min(mine, static_cast<int>(i));
    }
    publish_first(mine, first);
}

// v[i] != v[tmap[i]] (bit patterns apart from +-0: the host's creation check
// compares with != too; a NaN is caught by the finite check before this one)
__global__ void __launch_bounds__(kVT)
k_first_asymmetric(int n, const double* __restrict__ v, const int* __restrict__ tmap, int* __restrict__ first) {
    const long stride = static_cast<long>(gridDim.x) * kVT;
    int mine = INT_MAX;
    for (long i = static_cast<long>(blockIdx.x) * kVT + threadIdx.x; i < n; i += stride)
        if (v[i] != v[tmap[i]]) mine = min(mine, static_cast<int>(i));
    publish_first(mine, first);
}

// dst[j][i] = max(src[j][i], floor) for the four vectors of J, vector j by the
// blocks of blockIdx.y = j: one launch for x, y, w, z
template <bool WIDE>
__global__ void __launch_bounds__(kVT)
k_clamp_copy4(ClampJobs J, double floor) {
    const int j = blockIdx.y, n = J.len[j];
    const double* __restrict__ src = J.src[j];
    double* __restrict__ dst = J.dst[j];
    const long stride = static_cast<long>(gridDim.x) * kVT;
    const long t = static_cast<long>(blockIdx.x) * kVT + threadIdx.x;
    if (WIDE) {
        const int n2 = n >> 1;
        for (long g = t; g < n2; g += stride) {
            double2 a = reinterpret_cast<const double2*>(src)[g];
            a.x = fmax(a.x, floor);
            a.y = fmax(a.y, floor);
            reinterpret_cast<double2*>(dst)[g] = a;
        }
        if ((n & 1) && t == 0) dst[n - 1] = fmax(src[n - 1], floor);
    } else {
        for (long i = t; i < n; i += stride) dst[i] = fmax(src[i], floor);
    }
}

}  // namespace

void launch_gather_map(int n, const int* map, const double* src, double* dst, hipStream_t st) {
    if (n <= 0) return;
    if (aligned16(map) && aligned16(dst))
        hipLaunchKernelGGL(k_gather_map<true>, dim3(grid_for((n + 3) / 4)), dim3(kVT), 0, st, n, map, src, dst);
    else
        hipLaunchKernelGGL(k_gather_map<false>, dim3(grid_for(n)), dim3(kVT), 0, st, n, map, src, dst);
    IPO_HIP_CHECK(hipGetLastError());
}

template <int KIND>
static void launch_first_bad(int n, const double* v, int* first, hipStream_t st) {
    if (n <= 0) return;
    if (aligned16(v))
        hipLaunchKernelGGL((k_first_bad<KIND, true>), dim3(grid_for((n + 1) / 2)), dim3(kVT), 0, st, n, v, first);
    else
        hipLaunchKernelGGL((k_first_bad<KIND, false>), dim3(grid_for(n)), dim3(kVT), 0, st, n, v, first);
    IPO_HIP_CHECK(hipGetLastError());
}

void launch_first_nonfinite(int n, const double* v, int* first, hipStream_t st) { launch_first_bad<0>(n, v, first, st); }
void launch_first_nonpositive(int n, const double* v, int* first, hipStream_t st) { launch_first_bad<1>(n, v, first, st); }

void launch_first_asymmetric(int n, const double* v, const int* tmap, int* first, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_first_asymmetric, dim3(grid_for(n)), dim3(kVT), 0, st, n, v, tmap, first);
    IPO_HIP_CHECK(hipGetLastError());
}

void launch_clamp_copy4(const ClampJobs& J, double floor, hipStream_t st) {
    int nmax = 0;
    bool wide = true;
    for (int j = 0; j < 4; j++) {
        nmax = std::max(nmax, J.len[j]);
        wide = wide && aligned16(J.src[j]) && aligned16(J.dst[j]);
    }
    if (nmax <= 0) return;
    if (wide)
        hipLaunchKernelGGL(k_clamp_copy4<true>, dim3(grid_for((nmax + 1) / 2), 4), dim3(kVT), 0, st, J, floor);
    else
        hipLaunchKernelGGL(k_clamp_copy4<false>, dim3(grid_for(nmax), 4), dim3(kVT), 0, st, J, floor);
    IPO_HIP_CHECK(hipGetLastError());
}

}  // namespace ipo
