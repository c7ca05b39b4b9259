// gol-mi355x: step_signature<K, ROWS, BOUNDED> -- step_census that also hashes every generation it computes, and the
// two small kernels of signature mode (k_signature, k_board_diff), for gfx950 (CDNA4).
//
// A temporal-blocked pass keeps generations 1 .. K - 1 in registers only, so a hash of each generation can be taken
// nowhere but here.  The hash is the board signature of gol/signature.hpp: a wrapping sum over the words of
//     E * (rho(row) * gam(2 word)) + O * (rho(row) * gam(2 word + 1))
// with E / O the word's even / odd cells, the two VGPRs every level's output already lies in.  The census kernel's
// ownership masks give each level's output masked to the cells the lane owns, once per generation; per word and
// level the signature adds
//     ka = rho * gam_e;  kb = rho * gam_o                      (2 v_mul_lo_u32)
//     p = (u64)E' * ka + (u64)O' * kb                          (2 v_mad_u64_u32)
//     sig[l] += p                                              (1 ds_add_u64, no return)
// to the census kernel's 2 v_bitop3 + 2 v_bcnt.  The K accumulators sig[l] of a lane live in LDS, not in
// registers: K aligned VGPR pairs on top of the census kernel's 209-217 VGPRs put K = 6 and 8 past the 256 of two
// waves per SIMD (the allocator spilled 2-34 registers, which variants did changed with every edit), while the LDS
// pipe is idle in this kernel: 8 bytes per lane, level and row against some 70 VALU instructions.  A lane adds only
// to its own K slots (slot l of thread t at l * block + t: consecutive lanes, consecutive banks), zeroes them itself
// and reads them back itself, so there is no barrier anywhere; the block takes K * 2 KiB.  An owned row is a row of the tile, so its global row is
// grow0 + t with no wrap and an owned word's global index is gword0 + col; a lane keeps its two gam values for the
// whole wave.  In the one-row0 runner rho is wave-uniform: scalar work (s_mul_i32, shifts), and the compiler computes
// one rho per distinct row of a row triple (levels l and l + 1 of consecutive iterations output the same row).  In
// the per-lane runner (packed narrow segments, small boards) rho is computed per lane and level; that path's speed
// matters little.  Rows that are not owned get a key of whatever row number the arithmetic yields: their E' and O'
// are 0.
//
// The products ka and kb must be computed where they are used.  Left alone, the compiler notices that the levels of
// the three rows of a triple share their rows' keys, computes the 20 products of the triple's 10 rows up front and
// keeps them in VGPRs: K = 8 then needs 257-272 VGPRs and holds one wave per SIMD.  An empty asm statement on the
// row key (scalar runner) or on the row counter (per-lane runner) makes every use its own value.
//
// At the end of the wave each level's count (u32) and signature (u64) are summed over the lanes and one lane adds
// them to the level's slot with two 64-bit atomics.  A generation's slot is kSigSlotWords words: kSigStripes
// partial counts, then kSigStripes partial signatures, each on a 128-byte line of its own (the host adds them up); a
// wave adds into stripe  wave id mod kSigStripes.  (Atomics on one line complete one after the other; the census
// kernel's header tells what packed slots cost.)
//
// The kernel is the streaming wave of rule_runner.hpp (the gates, the level loop, the runner, the edge masks, the
// ownership masks of step_census and the choice between scalar and per-lane row tests and keys) with the count and
// the hash as its policy.  Plans, StepParams, loads and stores are step_rule's.
//
// slots (the slot of the pass's first generation) == nullptr skips the atomics (uniformly): the engine's init-time
// timing launches.
//
// Depths K = 1 .. 8, both row modes, both boundaries; registers: docs/PERFORMANCE.md section 22.
#include "gol/signature.hpp"
#include "rule_launch.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED>
// (the second launch bound: at least two waves per SIMD, so at most 256 registers and none of them an AGPR copy)
__global__ __launch_bounds__(64 * kWavesPerBlock, 2) void step_signature(const u64* __restrict__ src, u64* __restrict__ dst,
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
        RuleRunner<K, ROWS, SigPolicy<K, MASK_UNI, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, &lds[0]);
        w.run();
        w.policy.finish(w.tally, wave, slots);
    } else {
        RuleRunner<K, ROWS, SigPolicy<K, MASK_LANE, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, &lds[0]);
        w.run();
        w.policy.finish(w.tally, wave, slots);
    }
}

const void* signature_kernel_of(Nbhd nbhd, int k, u32 flags, bool bounded) {
    if (nbhd != Nbhd::Moore) return nbhd_signature_kernel(nbhd, k, flags, bounded);
    return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
        return bounded ? (const void*)step_signature<K(), ROWS(), true> : (const void*)step_signature<K(), ROWS(), false>;
    });
}

// The signature of the board in memory: one thread per tile word (grid-stride), a block-level reduction as
// k_reduce_board's, one atomic per block.
__global__ __launch_bounds__(256) void k_signature(const u64* __restrict__ buf, i64 pitch, int R, i64 h, i64 nw, i64 w,
                                                   i64 grow0, i64 gword0, unsigned long long* __restrict__ out) {
    u64 sg = 0;
    const i64 n = h * nw;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const i64 r = e / nw, c = e - r * nw;
        sg += signature_word(grow0 + r, gword0 + c, buf[(r + R) * pitch + c + 1] & storage_mask(c, w));
    }
    for (int off = 32; off > 0; off >>= 1) sg += __shfl_down(sg, off, 64);
    __shared__ u64 ss[4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) ss[wv] = sg;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 a = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) a += ss[i];
        atomicAdd(&out[0], (unsigned long long)a);
    }
}

// The number of cells of the tile that differ between two boards of one layout: popcount of the masked XOR, a wave
// reduction, one atomic per wave.
__global__ __launch_bounds__(256) void k_board_diff(const u64* __restrict__ a, const u64* __restrict__ b, i64 pitch, int R,
                                                    i64 h, i64 nw, i64 w, unsigned long long* __restrict__ out) {
    u64 diff = 0;
    const i64 n = h * nw;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const i64 r = e / nw, c = e - r * nw;
        const i64 at = (r + R) * pitch + c + 1;
        diff += (u64)__popcll((a[at] ^ b[at]) & storage_mask(c, w));
    }
    for (int off = 32; off > 0; off >>= 1) diff += __shfl_down(diff, off, 64);
    if ((threadIdx.x & 63) == 0 && diff != 0) atomicAdd(&out[0], (unsigned long long)diff);
}

unsigned reduce_grid(i64 n) {
    i64 g = ceil_div(n, 256);
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

int max_signature_depth(Nbhd) { return kMaxRuleDepth; }

int signature_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd) {
    return blocks_per_cu(signature_kernel_of(nbhd, k, flags, bounded));
}

void launch_step_signature(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src,
                           u64* dst, const LaneDesc* plan, i64 n_waves, const StepParams& p, u64* slots, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_signature has no seam-reading variant (sub-tiles do not run signature mode)");
    check_rule_masks("step_signature", rule);
    check_place("step_signature", place);
    check_tile_cols("step_signature", tile_cols, p);
    const void* f = signature_kernel_of(rule.nbhd, k, p.flags, bounded);
    if (!f) throw Error(strprintf("no signature kernel instantiated for depth %d (1..%d)", k, kMaxRuleDepth));
    launch_generic("signature", f, rule, src, dst, plan, n_waves, p, s, tile_args(&place, tile_cols, p), slots);
}

void launch_signature(const u64* buf, const Layout& L, i64 grow0, i64 gword0, u64* out, hipStream_t s) {
    hipLaunchKernelGGL(k_signature, dim3(reduce_grid(L.h * L.nw)), dim3(256), 0, s, buf, L.pitch, L.R, L.h, L.nw, L.w, grow0,
                       gword0, (unsigned long long*)out);
}

void launch_board_diff(const u64* a, const u64* b, const Layout& L, u64* out, hipStream_t s) {
    hipLaunchKernelGGL(k_board_diff, dim3(reduce_grid(L.h * L.nw)), dim3(256), 0, s, a, b, L.pitch, L.R, L.h, L.nw, L.w,
                       (unsigned long long*)out);
}

}  // namespace hipk
}  // namespace gol
