// gol-mi355x: step_signature_nbhd<K, ROWS, BOUNDED> -- step_signature (signature_kernel.hip) on the von Neumann and
// hexagonal neighbourhoods for gfx950 (CDNA4): the same streaming wave and signature policy with the gates of
// nbhd_gates.hpp.  Depths, row modes, boundaries, plans, StepParams, loads, stores, LDS and the slots are
// step_signature's.
//
// Registers: docs/PERFORMANCE.md section 24.
#include "nbhd_gates.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED, class Gates>
// (the second launch bound: at least two waves per SIMD, as step_signature)
__global__ __launch_bounds__(64 * kWavesPerBlock, 2) void step_signature_nbhd(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                            const LaneDesc* __restrict__ plan, StepParams p,
                                                                            RuleMasks rm, TileArgs ta, u64* __restrict__ slots) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    __shared__ unsigned long long lds[K * 64 * kWavesPerBlock];  // the lanes' signature accumulators (no barrier: each its own)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, SigPolicy<K, MASK_UNI, BOUNDED>, Gates> w(src, dst, d, nrows, p, wave, Gates(rm), ta, &lds[0]);
        w.run();
        w.policy.finish(w.tally, wave, slots);
    } else {
        RuleRunner<K, ROWS, SigPolicy<K, MASK_LANE, BOUNDED>, Gates> w(src, dst, d, nrows, p, wave, Gates(rm), ta, &lds[0]);
        w.run();
        w.policy.finish(w.tally, wave, slots);
    }
}

}  // namespace

const void* nbhd_signature_kernel(Nbhd nbhd, int k, u32 flags, bool bounded) {
    return nbhd_kernel_of(nbhd, [&](auto g) {
        using G = typename decltype(g)::type;
        return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
            return bounded ? (const void*)step_signature_nbhd<K(), ROWS(), true, G>
                           : (const void*)step_signature_nbhd<K(), ROWS(), false, G>;
        });
    });
}

}  // namespace hipk
}  // namespace gol
