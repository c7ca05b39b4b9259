// gol-mi355x: step_rule_bounded_nbhd<K> -- step_rule_bounded (rule_bounded_kernel.hip) on the von Neumann and
// hexagonal neighbourhoods for gfx950 (CDNA4): the same streaming wave and edge policy with the gates of
// nbhd_gates.hpp.  Depths, row modes, plans, StepParams, loads and stores are step_rule's.
//
// Registers: docs/PERFORMANCE.md section 24.
#include "nbhd_gates.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, class Gates>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_rule_bounded_nbhd(const u64* __restrict__ src,
                                                                               u64* __restrict__ dst,
                                                                               const LaneDesc* __restrict__ plan,
                                                                               StepParams p, RuleMasks rm, TileArgs ta) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, EdgePolicy<K, MASK_UNI>, Gates> w(src, dst, d, nrows, p, wave, Gates(rm), ta);
        w.run();
    } else {
        RuleRunner<K, ROWS, EdgePolicy<K, MASK_LANE>, Gates> w(src, dst, d, nrows, p, wave, Gates(rm), ta);
        w.run();
    }
}

}  // namespace

const void* nbhd_bounded_kernel(Nbhd nbhd, int k, u32 flags) {
    return nbhd_kernel_of(nbhd, [&](auto g) {
        using G = typename decltype(g)::type;
        return kernel_of(k, flags, [](auto K, auto ROWS) { return (const void*)step_rule_bounded_nbhd<K(), ROWS(), G>; });
    });
}

}  // namespace hipk
}  // namespace gol
