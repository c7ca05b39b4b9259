// gol-mi355x: step_rule<K> -- the generic life-like-rule kernel for gfx950 (CDNA4).
//
// One kernel for all 2^17 B0-free rules B.../S... (rule.hpp): the rule's two 9-bit masks are run-time,
// wave-uniform kernel arguments.  It is the streaming wave of rule_runner.hpp (the rule gates, the level loop and
// the runner, shared with step_rule_bounded, step_census and step_signature; the header tells what is
// step_temporal's and states the invariant that lets validate_plan cover these kernels) with no policy: nothing
// happens to a level's output but the next level.
//
// Registers: K = 8 takes 173 VGPRs (wrap rows; 172 with ghost rows), past the 168 of three waves per SIMD:
// step_rule<8> runs at 2 waves per SIMD, no spills (step_temporal<8>: 163, 3 waves).  K <= 7 take 155 or
// fewer (3 waves or more).  Measured: docs/PERFORMANCE.md section 18.
#include "rule_launch.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_rule(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                  const LaneDesc* __restrict__ plan, StepParams p,
                                                                  RuleMasks rm) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    RuleRunner<K, ROWS, NoPolicy> w(src, dst, d, nrows, p, wave, RuleGates(rm));
    w.run();
}

const void* rule_kernel_of(Nbhd nbhd, int k, u32 flags) {
    if (nbhd != Nbhd::Moore) return nbhd_rule_kernel(nbhd, k, flags);
    return kernel_of(k, flags, [](auto K, auto ROWS) { return (const void*)step_rule<K(), ROWS()>; });
}

}  // namespace

bool rule_depth_supported(int k, Nbhd nbhd) { return k >= 1 && k <= max_rule_depth(nbhd); }

int max_rule_depth(Nbhd) { return kMaxRuleDepth; }

int rule_blocks_per_cu(int k, u32 flags, Nbhd nbhd) { return blocks_per_cu(rule_kernel_of(nbhd, k, flags)); }

void launch_step_rule(int k, const Rule& rule, const u64* src, u64* dst, const LaneDesc* plan, i64 n_waves,
                      const StepParams& p, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_rule has no seam-reading variant (sub-tiles run B3/S23 only)");
    check_rule_masks("step_rule", rule);
    const void* f = rule_kernel_of(rule.nbhd, k, p.flags);
    if (!f) throw Error(strprintf("no rule kernel instantiated for depth %d", k));
    launch_generic("rule", f, rule, src, dst, plan, n_waves, p, s);
}

}  // namespace hipk
}  // namespace gol
