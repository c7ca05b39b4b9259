// gol-mi355x: step_envelope_nbhd<K, ROWS, BOUNDED> -- step_envelope (envelope_kernel.hip) on the von Neumann and
// hexagonal neighbourhoods for gfx950 (CDNA4): the same streaming wave and envelope policy with the gates of
// nbhd_gates.hpp.  Depths, row modes, boundaries, plans, StepParams, loads, stores and the envelope buffer are
// step_envelope's.
//
// Registers: docs/PERFORMANCE.md section 28.
#include "nbhd_gates.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED, class Gates>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_envelope_nbhd(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                       const LaneDesc* __restrict__ plan, StepParams p,
                                                                       RuleMasks rm, TileArgs ta, EnvelopeArgs ea) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, EnvelopePolicy<K, MASK_UNI, BOUNDED>, Gates> w(src, dst, d, nrows, p, wave, Gates(rm), ta, ea);
        w.run();
    } else {
        RuleRunner<K, ROWS, EnvelopePolicy<K, MASK_LANE, BOUNDED>, Gates> w(src, dst, d, nrows, p, wave, Gates(rm), ta, ea);
        w.run();
    }
}

}  // namespace

const void* nbhd_envelope_kernel(Nbhd nbhd, int k, u32 flags, bool bounded) {
    return nbhd_kernel_of(nbhd, [&](auto g) {
        using G = typename decltype(g)::type;
        return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
            return bounded ? (const void*)step_envelope_nbhd<K(), ROWS(), true, G> : (const void*)step_envelope_nbhd<K(), ROWS(), false, G>;
        });
    });
}

}  // namespace hipk
}  // namespace gol
