// gol-mi355x: step_rule_nbhd<K> -- step_rule (rule_kernel.hip) on the von Neumann and hexagonal neighbourhoods for
// gfx950 (CDNA4): the same streaming wave with the gates of nbhd_gates.hpp (the header counts them).  Depths, row
// modes, plans, StepParams, loads and stores are step_rule's.
//
// Registers: docs/PERFORMANCE.md section 24.
#include "nbhd_gates.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, class Gates>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_rule_nbhd(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                       const LaneDesc* __restrict__ plan, StepParams p,
                                                                       RuleMasks rm) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    RuleRunner<K, ROWS, NoPolicy, Gates> w(src, dst, d, nrows, p, wave, Gates(rm));
    w.run();
}

}  // namespace

const void* nbhd_rule_kernel(Nbhd nbhd, int k, u32 flags) {
    return nbhd_kernel_of(nbhd, [&](auto g) {
        using G = typename decltype(g)::type;
        return kernel_of(k, flags, [](auto K, auto ROWS) { return (const void*)step_rule_nbhd<K(), ROWS(), G>; });
    });
}

}  // namespace hipk
}  // namespace gol
