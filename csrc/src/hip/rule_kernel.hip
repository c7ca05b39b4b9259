// gol-mi355x: step_rule<K> -- the generic life-like-rule kernel for gfx950 (CDNA4).
//
// One kernel for all 2^17 B0-free rules B.../S... (rule.hpp): the rule's two 9-bit masks are run-time,
// wave-uniform kernel arguments (an argument of their own: StepParams, and with it the kernarg layout of
// every other kernel, is unchanged).  Everything but the last gates of a level is step_temporal's
// (step_kernels.hip): the same plans (LaneDesc: 62 output + 2 halo lanes per wave, trash slots for lanes that
// store nothing), the same StepParams, the same streaming wave (RuleRunner below: wave_runner.hpp's row
// prefetch and ROWS_GHOST / ROWS_WRAP load stream), the same split word format, hsum_split, DPP lane moves
// and v_bitop3_b32 adders, the same register ring (three slots of s0, s1, x per level and half; no extra
// plane lives across rows).
//
// INVARIANT (what makes the host-side validate_plan sufficient for this kernel too): step_rule<K> reads and
// writes exactly the rows and words step_temporal<K> reads and writes for the same plan and StepParams.  The
// loads, the stores and their addresses are those of WaveRunner<K, ROWS> (RuleRunner repeats them); the rule
// step (RuleStep below) only replaces the register arithmetic between a row's load and its store and touches
// no memory.
//
// Rule evaluation, per level and word half (v_bitop3_b32's truth table is an immediate, so a run-time rule
// cannot be folded into LUTs):
//   * the four planes of T, the 3x3 sum INCLUDING the centre (0..9), from the ring's horizontal sums, 7 gates:
//       x0, cy, u0, u1 as in rule32;  t0 = x0,  t1 = cy ^ u0,  t2 = u1 ^ (cy & u0),  t3 = u1 & cy & u0
//   * F(T, x) = x ? survive[T - 1] : birth[T] as a mux tree over (t0, t1, t2, t3) whose leaves
//     leaf_T = x ? S[T-1] : B[T] select between two uniform all-ones / all-zeros words, 17 gates:
//       T = 0 needs no leaf (x = 1 is impossible, B0 is refused: the pair (0, 1) is t0 & leaf_1), T = 9 has
//       x = 1 (the pair (8, 9) is x ? (t0 ? S8 : S7) : B8): 7 leaves + 1 and + 2 + 3 pair muxes + 4 tree muxes.
//   24 v_bitop3 per word half and level against rule32's 7; with the 4 of hsum_split 28 against 11.
//   (A decode-and-accumulate form, F = xor of coefficient & monomial over the 19 reachable (T, x), takes one
//   uniform operand per gate but 24 gates after the planes; the tree was kept for its count.)
//   A VOP3 instruction of this ISA generation reads one SGPR, and a leaf has two uniform operands: in the
//   K = 8 steady loop the compiler keeps one operand of each leaf in a VGPR across the rows (about ten
//   registers) instead of a v_mov_b32 per leaf: 1386 VALU per three rows, 1248 of them v_bitop3 (4 of the 56
//   per row and level are folded), 12-14 v_mov_b32, no s_nop, against step_temporal<8>'s 562.
//
// Registers: K = 8 takes 173 VGPRs (wrap rows; 172 with ghost rows), past the 168 of three waves per SIMD:
// step_rule<8> runs at 2 waves per SIMD, no spills (step_temporal<8>: 163, 3 waves).  K <= 7 take 155 or
// fewer (3 waves or more).  Measured: docs/PERFORMANCE.md section 18.
//
// Depths K = 1 .. 8 are instantiated: every remainder of a superstep is one pass.
#include "gol/bits.hpp"
#include "gol/hip_kernels.hpp"
#include "stencil_device.hpp"
#include "wave_runner.hpp"

namespace gol {
namespace hipk {

namespace {

constexpr unsigned kLutMux = 0xCA;   // a ? b : c
constexpr unsigned kLutAnd3 = 0x80;  // a & b & c
constexpr unsigned kLutAnd2 = 0xC0;  // a & b
constexpr unsigned kLutXor2 = 0x3C;  // a ^ b
constexpr unsigned kLutXorAnd = lut3([](unsigned a, unsigned b, unsigned c) { return a ^ (b & c); });
static_assert(kLutMux == lut3([](unsigned a, unsigned b, unsigned c) { return (a & b) | (~a & c); }), "mux LUT");
static_assert(kLutAnd3 == lut3([](unsigned a, unsigned b, unsigned c) { return a & b & c; }), "and3 LUT");
static_assert(kLutAnd2 == lut3([](unsigned a, unsigned b, unsigned) { return a & b; }), "and2 LUT");
static_assert(kLutXor2 == lut3([](unsigned a, unsigned b, unsigned) { return a ^ b; }), "xor2 LUT");

struct RuleMasks {
    u32 birth, survive;
};

// The rule step of the streaming wave: the uniform leaf words of the rule (all ones / all zeros), and the
// level pipeline with the generic finish.
struct RuleStep {
    u32 B[9];  // B[c]: a dead cell with c neighbours is born   (B[0] is 0: refused on the host)
    u32 S[9];  // S[c]: a live cell with c neighbours survives

    __device__ __forceinline__ explicit RuleStep(const RuleMasks& m) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            B[c] = 0u - ((m.birth >> c) & 1u);
            S[c] = 0u - ((m.survive >> c) & 1u);
        }
    }

    // leaf_T(x) = x ? S[T - 1] : B[T]
    template <int T>
    __device__ __forceinline__ u32 leaf(u32 x) const {
        return b3<kLutMux>(x, S[T - 1], B[T]);
    }

    // next state of 32 cells from the three rows' horizontal sums (a, b, c) and the centre row x
    __device__ __forceinline__ u32 rule(u32 a0, u32 a1, u32 b0, u32 b1, u32 c0, u32 c1, u32 x) const {
        const u32 t0 = b3<kLutXor3>(a0, b0, c0);
        const u32 cy = b3<kLutMaj>(a0, b0, c0);
        const u32 u0 = b3<kLutXor3>(a1, b1, c1);
        const u32 u1 = b3<kLutMaj>(a1, b1, c1);
        const u32 t1 = b3<kLutXor2>(cy, u0, u0);
        const u32 t2 = b3<kLutXorAnd>(u1, cy, u0);
        const u32 t3 = b3<kLutAnd3>(u1, cy, u0);
        const u32 m01 = b3<kLutAnd2>(t0, leaf<1>(x), x);
        const u32 m23 = b3<kLutMux>(t0, leaf<3>(x), leaf<2>(x));
        const u32 m45 = b3<kLutMux>(t0, leaf<5>(x), leaf<4>(x));
        const u32 m67 = b3<kLutMux>(t0, leaf<7>(x), leaf<6>(x));
        const u32 s89 = b3<kLutMux>(t0, S[8], S[7]);  // T = 9 has a live centre
        const u32 m89 = b3<kLutMux>(x, s89, B[8]);
        const u32 q0 = b3<kLutMux>(t1, m23, m01);
        const u32 q1 = b3<kLutMux>(t1, m67, m45);
        const u32 lo = b3<kLutMux>(t2, q1, q0);
        return b3<kLutMux>(t3, m89, lo);  // T >= 8: t1 = t2 = 0
    }

    // Push one row through the K levels: advance() of stencil_device.hpp without the pair mode, with rule()
    // as the finish.  Same ring, same slots, same fill-phase guards.
    template <int K, int PH, bool GUARD>
    __device__ __forceinline__ bool advance(Pipe<K>& P, u32& lo, u32& hi, int i) const {
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (GUARD && i < 2 * l) return false;
            const int s = (PH + l) % 3;   // slot of the arriving row
            const int sp = (s + 2) % 3;   // previous row (centre of the output)
            const int spp = (s + 1) % 3;  // two rows back
            hsum_split(lo, hi, P.s0[l][s][0], P.s1[l][s][0], P.s0[l][s][1], P.s1[l][s][1]);
            P.x[l][s][0] = lo;
            P.x[l][s][1] = hi;
            if (GUARD && i < 2 * l + 2) return false;
            lo = rule(P.s0[l][spp][0], P.s1[l][spp][0], P.s0[l][sp][0], P.s1[l][sp][0], P.s0[l][s][0], P.s1[l][s][0],
                      P.x[l][sp][0]);
            hi = rule(P.s0[l][spp][1], P.s1[l][spp][1], P.s0[l][sp][1], P.s1[l][sp][1], P.s0[l][s][1], P.s1[l][s][1],
                      P.x[l][sp][1]);
        }
        return true;
    }
};

// The streaming wave of step_rule: WaveRunner of wave_runner.hpp (step_temporal's) with the rule step in
// place of advance(), copied rather than shared.  (Sharing it through a step-policy template parameter whose
// default reproduced step_temporal's instantiations was tried first: the gfx950 code of step_kernels.hip then
// differed from the parent's in register allocation, so the existing runner stays untouched;
// docs/PERFORMANCE.md "Life-like rules".)  What is kept, line for line: the constructor's addresses (load
// stream from row row0 - K, store pointer or trash slot, strides), next_row's ROWS_WRAP select, the prefetch
// depth prefetch_rows<K>() and with it the rows read past a segment's last input row (3 or 6: the engine's
// slack rows), one store per row from row 2K on.  What is left out: ROWS_SEAM (sub-tiles run B3/S23 only) and
// the two-triple steady loop (at K = 7 it took 271 registers here against 155 with the one-triple loop).
template <int K, int ROWS>
struct RuleRunner {
    static_assert(ROWS == ROWS_GHOST || ROWS == ROWS_WRAP, "step_rule reads ghost rows or wraps");
    static constexpr int D = prefetch_rows<K>();
    const RuleStep step;
    const StepParams& p;
    const LaneDesc& d;
    const int n;   // row iterations: nrows + 2K
    const i64 hp;  // h * pitch
    const uint2* ld;
    uint2* st;
    i64 st_stride;  // pitch for output lanes, 0 for halo/idle lanes (they write a trash slot)
    int lrow;       // tile row of the next load (ROWS_WRAP; wave-uniform)
    uint2 pf[D];
    Pipe<K> P;

    __device__ __forceinline__ void next_row() {
        ld += p.pitch;
        if (ROWS == ROWS_WRAP) {  // rows are periodic: row h is row 0 (branch-free select)
            ++lrow;
            const bool w = lrow == p.h;
            lrow = w ? 0 : lrow;
            ld = w ? ld - hp : ld;
        }
    }

    __device__ __forceinline__ RuleRunner(const u64* src, u64* dst, const LaneDesc& d_, int nrows, const StepParams& p_,
                                          i64 wave_id, const RuleStep& step_)
        : step(step_), p(p_), d(d_), n(nrows + 2 * K), hp((i64)p_.h * p_.pitch) {
        lrow = d.row0 - K;
        if (ROWS == ROWS_WRAP && lrow < 0) lrow += p.h;
        ld = reinterpret_cast<const uint2*>(src + (i64)(lrow + p.R) * p.pitch + (d.col + 1));
        // every lane stores every row; halo/idle lanes write a trash word of their own (wave_runner.hpp)
        const bool out = d.flags & LANE_STORE;
        st = out ? reinterpret_cast<uint2*>(dst + (i64)(d.row0 + p.R) * p.pitch + (d.col + 1))
                 : reinterpret_cast<uint2*>(p.trash + ((i64)(wave_id & (kTrashWaves - 1)) * 64 + (threadIdx.x & 63)));
        st_stride = out ? p.pitch : 0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            ROW_LOAD_INTO(pf[j]);
            next_row();
        }
    }

    // Next input row (lo, hi) in order.
    template <int PH>
    __device__ __forceinline__ void fetch(u32& lo, u32& hi) {
        uint2 x;
        if constexpr (D == 3) {
            x = pf[PH];
            ROW_LOAD_INTO(pf[PH]);  // prefetch 3 rows ahead (the allocation has slack rows past the halo)
        } else {
            x = pf[0];  // a queue of D rows (the shift is register renaming in the unrolled code)
#pragma unroll
            for (int j = 0; j + 1 < D; ++j) pf[j] = pf[j + 1];
            ROW_LOAD_INTO(pf[D - 1]);
        }
        next_row();
        lo = x.x;
        hi = x.y;
    }

    template <int PH, bool GUARD>
    __device__ __forceinline__ void compute_store(u32 lo, u32 hi, int i) {
        if (!step.template advance<K, PH, GUARD>(P, lo, hi, i)) return;
        *st = make_uint2(lo, hi);
        st += st_stride;
    }

    template <int PH, bool GUARD>
    __device__ __forceinline__ void body(int i) {
        if (GUARD && i >= n) return;
        u32 lo, hi;
        fetch<PH>(lo, hi);
        compute_store<PH, GUARD>(lo, hi, i);
    }

    __device__ __forceinline__ void run() {
        constexpr int i0 = ((2 * K + 2) / 3) * 3;  // first multiple of 3 at which the pipeline is full
        int i = 0;
        for (; i < i0; i += 3) {
            body<0, true>(i);
            body<1, true>(i + 1);
            body<2, true>(i + 2);
        }
        if constexpr (D == 6) {
            // shallow (memory-bound) passes: six loads in flight per wave (wave_runner.hpp)
#define RULE_ROW6_STEP(J)                                     \
    compute_store<(J) % 3, false>(pf[J].x, pf[J].y, i + (J)); \
    ROW_LOAD_INTO(pf[J]);                                     \
    next_row();                                               \
    __builtin_amdgcn_sched_barrier(0);
            for (; i + 6 <= n; i += 6) {
                RULE_ROW6_STEP(0) RULE_ROW6_STEP(1) RULE_ROW6_STEP(2) RULE_ROW6_STEP(3) RULE_ROW6_STEP(4) RULE_ROW6_STEP(5)
            }
#undef RULE_ROW6_STEP
            // fewer than six rows left, in pf[0..] in order
            if (i < n) compute_store<0, false>(pf[0].x, pf[0].y, i);
            if (i + 1 < n) compute_store<1, false>(pf[1].x, pf[1].y, i + 1);
            if (i + 2 < n) compute_store<2, false>(pf[2].x, pf[2].y, i + 2);
            if (i + 3 < n) compute_store<0, false>(pf[3].x, pf[3].y, i + 3);
            if (i + 4 < n) compute_store<1, false>(pf[4].x, pf[4].y, i + 4);
        } else {
            for (; i + 3 <= n; i += 3) {
                // hoist the whole next triple's loads above this triple's compute
                const uint2 x0 = pf[0], x1 = pf[1], x2 = pf[2];
                ROW_LOAD_INTO(pf[0]);
                next_row();
                ROW_LOAD_INTO(pf[1]);
                next_row();
                ROW_LOAD_INTO(pf[2]);
                next_row();
                __builtin_amdgcn_sched_barrier(0);
                compute_store<0, false>(x0.x, x0.y, i);
                compute_store<1, false>(x1.x, x1.y, i + 1);
                compute_store<2, false>(x2.x, x2.y, i + 2);
            }
            if (i < n) body<0, false>(i);
            if (i + 1 < n) body<1, false>(i + 1);
        }
    }
};

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
    RuleRunner<K, ROWS> w(src, dst, d, nrows, p, wave, RuleStep(rm));
    w.run();
}

template <int K>
const void* rule_kernel_for(u32 flags) {
    return (flags & STEP_WRAP_Y) ? (const void*)step_rule<K, ROWS_WRAP> : (const void*)step_rule<K, ROWS_GHOST>;
}

#define FOR_EACH_RULE_DEPTH(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

const void* rule_kernel_of(int k, u32 flags) {
    switch (k) {
#define DEPTH_CASE(K) \
    case K:           \
        return rule_kernel_for<K>(flags);
        FOR_EACH_RULE_DEPTH(DEPTH_CASE)
#undef DEPTH_CASE
        default:
            return nullptr;
    }
}

}  // namespace

bool rule_depth_supported(int k) { return k >= 1 && k <= max_rule_depth(); }

int max_rule_depth() { return 8; }

int rule_blocks_per_cu(int k, u32 flags) {
    const void* f = rule_kernel_of(k, flags);
    int nb = 0;
    if (!f || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 64 * kWavesPerBlock, 0) != hipSuccess || nb < 1) return 1;
    return std::min(nb, 32 / kWavesPerBlock);
}

void launch_step_rule(int k, const Rule& rule, const u64* src, u64* dst, const LaneDesc* plan, i64 n_waves,
                      const StepParams& p, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_rule has no seam-reading variant (sub-tiles run B3/S23 only)");
    if ((rule.birth & 1u) || rule.birth > 0x1FFu || rule.survive > 0x1FFu)
        throw Error("step_rule: rule masks outside B1..8 / S0..8 (B0 is out of scope)");
    const void* f = rule_kernel_of(k, p.flags);
    if (!f) throw Error(strprintf("no rule kernel instantiated for depth %d", k));
    const dim3 grid((unsigned)(n_waves / kWavesPerBlock)), block(64 * kWavesPerBlock);
    StepParams pp = p;
    if (!pp.trash) pp.trash = trash_of_current_device();
    RuleMasks rm{rule.birth, rule.survive};
    void* args[] = {(void*)&src, (void*)&dst, (void*)&plan, (void*)&pp, (void*)&rm};
    hipError_t e = hipLaunchKernel(f, grid, block, args, 0, s);
    if (e != hipSuccess) throw Error(strprintf("rule kernel launch failed: %s", hipGetErrorString(e)));
}

}  // namespace hipk
}  // namespace gol
