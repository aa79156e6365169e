// Microbenchmark of the dense tail's deferred trailing update (visit_tile512,
// kkt_dense.hip; developer tool, not part of the library): G workgroups each
// apply a chunk of `chunk` blocks to their own 64 x 64 tile of an nt x nt
// tail, with the LDS footprint of the fused step kernel (one workgroup per
// CU) or of the visit alone (two per CU); "same" makes every workgroup read
// the operands of one tile (cache-resident: the compute + LDS bound).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off \
//         [-DIPO_VISIT_STAMPS] -I linear-programming-vanderbei_amd/csrc tools/ubench_visit.hip \
//         linear-programming-vanderbei_amd/csrc/kkt_schedule.cpp -o tools/ubench_visit
//   tools/ubench_visit [nt]                 (the table below)
//   tools/ubench_visit nt mode chunk G reps (one configuration: for counter passes)
#include "../linear-programming-vanderbei_amd/csrc/kkt_dense.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("%s: %s\n", #x, hipGetErrorString(e_)); std::exit(1); } } while (0)

namespace ipo {

// workgroup g -> tile g of the lower triangle of block columns >= c0 (or
// tile (c0 + 1, c0) for all: same); offd: strictly below the diagonal only
template <size_t LDSB>
__global__ void __launch_bounds__(PNT) k_visit_bench(PlanView p, TailView tv, int c0, int b0, int b1, int same,
                                                     int offd) {
    __shared__ __attribute__((aligned(16))) char lds[LDSB];
    int tile = blockIdx.x, c = c0;
    if (!same)
        while (tile >= tv.ntb - c - offd) { tile -= tv.ntb - c - offd; c++; }
    else
        tile = 0;
    if (c >= tv.ntb) return;
    visit_tile512(p, tv, c + offd + tile, c, b0, b1, *reinterpret_cast<SyrkLds*>(lds));
}

}  // namespace ipo

int main(int argc, char** argv) {
    const int nt = argc > 1 ? std::atoi(argv[1]) : 4441;
    const int ntb = (nt + 63) / 64;
    const size_t bytes = (size_t)nt * nt * sizeof(double);
    double *dS, *ddg, *ddsc;
    CK(hipMalloc(&dS, bytes)); CK(hipMalloc(&ddg, nt * 8)); CK(hipMalloc(&ddsc, nt * 8));
    std::vector<double> S((size_t)nt * nt);
    for (size_t i = 0; i < S.size(); i++) S[i] = 1e-3 * (double)((i * 2654435761u) % 1000) / 1000.0;
    std::vector<double> g(nt, 1.0);
    CK(hipMemcpy(dS, S.data(), bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(ddg, g.data(), nt * 8, hipMemcpyHostToDevice));
    CK(hipMemset(ddsc, 0, nt * 8));
    ipo::PlanView pv{};
    pv.dg = ddg; pv.dscale = ddsc; pv.tau = 1e-17;
    ipo::TailView tv{};
    tv.S = dS; tv.nt = nt; tv.ntb = ntb; tv.tc = 0;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int c0 = 20;        // columns 20.. : 50 + 49 + ... tiles available, blocks 0..19 as operands
    const int maxg = (ntb - c0) * (ntb - c0 + 1) / 2;
    std::printf("nt %d; visit of G tiles, chunk blocks each; us per launch (us per block)\n", nt);
    struct Mode { int same, big, offd; const char* what; };
    const Mode modes[] = {{0, 1, 0, "own operands, diagonal tiles included"},
                          {0, 1, 1, "own operands, below the diagonal only"},
                          {1, 1, 1, "every workgroup one off-diagonal tile's operands"},
                          {0, 0, 1, "own operands, below the diagonal, LDS of the visit alone"}};
    const bool one = argc > 5;
    const int one_mode = one ? std::atoi(argv[2]) : 0, one_chunk = one ? std::atoi(argv[3]) : 0,
              one_g = one ? std::atoi(argv[4]) : 0, one_reps = one ? std::atoi(argv[5]) : 20;
    for (const Mode& md : modes) {
        if (one && &md != &modes[one_mode]) continue;
        std::printf("%s:\n", md.what);
        for (int chunk : {1, 4, 8}) {
            if (one) chunk = one_chunk;
            std::printf("  chunk %d:", chunk);
            for (int G : {1, 64, 256, 384, 512}) {
                if (one) G = one_g;
                if (G > maxg) continue;
                auto launch = [&]() {
                    if (md.big)
                        hipLaunchKernelGGL((ipo::k_visit_bench<ipo::kTailStepLds>), dim3(G), dim3(ipo::PNT), 0, 0, pv, tv,
                                           c0, 0, chunk, md.same, md.offd);
                    else
                        hipLaunchKernelGGL((ipo::k_visit_bench<sizeof(ipo::SyrkLds)>), dim3(G), dim3(ipo::PNT), 0, 0, pv,
                                           tv, c0, 0, chunk, md.same, md.offd);
                };
                launch();
                CK(hipDeviceSynchronize());
                const int reps = one ? one_reps : 20;
                CK(hipEventRecord(e0, 0));
                for (int r = 0; r < reps; r++) launch();
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, e0, e1));
                const double us = 1e3 * ms / reps;
                std::printf("  G%d %.1f (%.2f)", G, us, us / chunk);
                if (one) break;
            }
            std::printf("\n");
            if (one) break;
        }
    }
#ifdef IPO_VISIT_STAMPS
    {
        long long st[8][16][6];
        CK(hipMemcpyFromSymbol(st, HIP_SYMBOL(ipo::g_vstamps), sizeof(st)));
        std::printf("workgroup 0 of the last launch, cycles from wave 0's first block start; slots per block: "
                    "0 start, 1 staged, 2 barrier, 3 next loads issued, 4 MFMA issued, 5 end barrier\n");
        const long long b0 = st[0][0][0];
        for (int w = 0; w < 8; w += 3) {
            std::printf("wave %d:\n", w);
            for (int b = 0; b < 8; b++) {
                std::printf("  block %d:", b);
                for (int sl = 0; sl < 6; sl++) std::printf(" %7lld", st[w][b][sl] - b0);
                std::printf("\n");
            }
        }
    }
#endif
    return 0;
}
