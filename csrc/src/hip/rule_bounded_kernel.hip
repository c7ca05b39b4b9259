// gol-mi355x: step_rule_bounded<K> -- step_rule (rule_kernel.hip) on a bounded board for gfx950 (CDNA4).
//
// A bounded board (Boundary::Dead) has no neighbours beyond its edges: every cell outside [0, H) x [0, W) of
// the GLOBAL board is dead in every generation.  A temporal-blocked pass runs K generations inside registers,
// so clearing the halos before the pass is not enough: a cell just outside the edge is born from inside cells
// at level 1 and feeds back at level 2.  This kernel masks the loaded row ("level 0") and the output of every
// level with the in-board cells of the word the lane streams.
//
// What is step_rule's, unchanged: the plans, StepParams (no kernarg layout moves), the streaming wave (load
// stream, prefetch depth, ROWS_GHOST / ROWS_WRAP, one store per row from row 2K on, trash slots), the split
// word format, hsum_split, the rule gates and the register ring.  RuleStep::rule and the runner are copied, not
// shared through a header: rule_kernel.hip and step_kernels.hip stay byte for byte what they were, and with them
// their gfx950 code (rule_kernel.hip tells how sharing a runner once changed the existing kernels' registers).
// So this kernel too reads and writes exactly the rows and words step_temporal<K> does for the same plan, and
// validate_plan covers it.  The engine builds bounded plans without x-wrap (halo lanes stream the ghost words,
// col = -1 or nw), so a lane's global word index tells whether it is outside the board.
//
// The masks (BoundArgs, one more kernel argument beside RuleMasks):
//   * column mask, per lane, formed once at kernel start from the global index of the lane's word: all ones
//     inside the board, the tail mask (split order) on the board's last word, zero beyond either edge;
//   * row mask, per level: the level-j value of row iteration i (j = 0 the loaded row, j = l + 1 the output of
//     level l) belongs to the unwrapped tile row  row0 - K + i - j,  and the loop counter i IS the unwrapped
//     row counter (lrow, the ROWS_WRAP load row, wraps several times per pass on a 1-, 2- or 3-row board; i does
//     not).  The row is on the board iff  (u32)(i - j - A) < span  with  A = row_lo - row0 + K,  row_lo the tile
//     row of global row 0 and span the board's rows.
//   A level's value is then  x & colmask & rowmask: one v_bitop3 (and3) per word half.
// row0 is a lane's segment's first row.  A wave that streams one segment (every full-width segment) has one
// row0: there A is made scalar with readfirstlane and the row mask costs s_sub + s_cmp + s_cselect per level,
// no VALU (UNI runner).  The planner packs several narrow segments of the same height, but of different rows,
// into one wave (plan.cpp pack_waves): such a wave keeps A per lane and pays v_sub + v_cmp + v_cndmask per
// level on top (the same source, A in a VGPR).  The kernel picks the runner per wave, uniformly.
// (A third runner without masks for waves that reach no edge was built and measured: slower, 32768^2 30.4 against
// 24.2 us/gen, 8192^2 5.35 against 4.70 -- three unrolled K = 8 loops in one kernel -- so it is not here.)
//
// Depths K = 1 .. 8, both row modes, as step_rule.
#include "gol/bits.hpp"
#include "gol/hip_kernels.hpp"
#include "stencil_device.hpp"
#include "wave_runner.hpp"

// A/B build (docs/PERFORMANCE.md "Bounded boards"): which rows of a K = 8 row triple a scheduling barrier follows
// (bit 0: the first, bit 1: the second).
#ifndef GOL_BOUNDED_ROW_BARRIERS
#define GOL_BOUNDED_ROW_BARRIERS 2
#endif

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

struct RuleMasks {
    u32 birth, survive;
};

// The board's edges as the kernel sees them (filled in by launch_step_rule_bounded from BoardEdges).
struct BoundArgs {
    i64 grow0;         // global row of tile row 0
    i64 grows;         // rows of the global board (H)
    i64 gword0;        // global word index of tile word 0
    i64 gwords;        // words per global row, ceil(W / 64)
    u32 tail_lo, tail_hi;  // valid cells of the last word, split order (even / odd columns)
};

// Row and column masks of one lane.  A is a scalar in the UNI runner (readfirstlane), a VGPR otherwise.
enum { MASK_UNI = 1, MASK_LANE = 2 };  // one row0 per wave (scalar row masks) / row0 per lane

template <int MASK>
struct EdgeMask {
    u32 col_lo, col_hi;
    int A;
    u32 span;

    // all ones when the level-j value of row iteration i (t = i - j) is a row of the board
    __device__ __forceinline__ u32 row(int t) const { return (u32)(t - A) < span ? ~0u : 0u; }
    __device__ __forceinline__ void apply(u32& lo, u32& hi, int t) const {
        const u32 r = row(t);
        lo = b3<kLutAnd3>(lo, col_lo, r);
        hi = b3<kLutAnd3>(hi, col_hi, r);
    }
};

// RuleStep of rule_kernel.hip (the rule's uniform leaf words and the generic finish), with the level outputs
// masked.
struct BoundedRuleStep {
    u32 B[9];
    u32 S[9];

    __device__ __forceinline__ explicit BoundedRuleStep(const RuleMasks& m) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            B[c] = 0u - ((m.birth >> c) & 1u);
            S[c] = 0u - ((m.survive >> c) & 1u);
        }
    }

    template <int T>
    __device__ __forceinline__ u32 leaf(u32 x) const {
        return b3<kLutMux>(x, S[T - 1], B[T]);
    }

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
        const u32 s89 = b3<kLutMux>(t0, S[8], S[7]);
        const u32 m89 = b3<kLutMux>(x, s89, B[8]);
        const u32 q0 = b3<kLutMux>(t1, m23, m01);
        const u32 q1 = b3<kLutMux>(t1, m67, m45);
        const u32 lo = b3<kLutMux>(t2, q1, q0);
        return b3<kLutMux>(t3, m89, lo);
    }

    // RuleStep::advance with the edge masks: the arriving row (lo, hi) is already masked (level 0, or the
    // previous level's masked output); the output of level l is centred on the row one iteration back per level.
    template <int K, int PH, bool GUARD, int MASK>
    __device__ __forceinline__ bool advance(Pipe<K>& P, u32& lo, u32& hi, int i, const EdgeMask<MASK>& em) const {
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (GUARD && i < 2 * l) return false;
            const int s = (PH + l) % 3;
            const int sp = (s + 2) % 3;
            const int spp = (s + 1) % 3;
            hsum_split(lo, hi, P.s0[l][s][0], P.s1[l][s][0], P.s0[l][s][1], P.s1[l][s][1]);
            P.x[l][s][0] = lo;
            P.x[l][s][1] = hi;
            if (GUARD && i < 2 * l + 2) return false;
            lo = rule(P.s0[l][spp][0], P.s1[l][spp][0], P.s0[l][sp][0], P.s1[l][sp][0], P.s0[l][s][0], P.s1[l][s][0],
                      P.x[l][sp][0]);
            hi = rule(P.s0[l][spp][1], P.s1[l][spp][1], P.s0[l][sp][1], P.s1[l][sp][1], P.s0[l][s][1], P.s1[l][s][1],
                      P.x[l][sp][1]);
            em.apply(lo, hi, i - (l + 1));
        }
        return true;
    }
};

// RuleRunner of rule_kernel.hip with the masks: the constructor's addresses, next_row, the prefetch and the
// loops are its, line for line; compute_store masks the loaded row before the levels.
template <int K, int ROWS, int MASK>
struct BoundedRunner {
    static_assert(ROWS == ROWS_GHOST || ROWS == ROWS_WRAP, "step_rule_bounded reads ghost rows or wraps");
    static constexpr int D = prefetch_rows<K>();
    const BoundedRuleStep step;
    const StepParams& p;
    const LaneDesc& d;
    const int n;   // row iterations: nrows + 2K
    const i64 hp;  // h * pitch
    EdgeMask<MASK> em;
    const uint2* ld;
    uint2* st;
    i64 st_stride;
    int lrow;
    uint2 pf[D];
    Pipe<K> P;

    __device__ __forceinline__ void next_row() {
        ld += p.pitch;
        if (ROWS == ROWS_WRAP) {
            ++lrow;
            const bool w = lrow == p.h;
            lrow = w ? 0 : lrow;
            ld = w ? ld - hp : ld;
        }
    }

    __device__ __forceinline__ BoundedRunner(const u64* src, u64* dst, const LaneDesc& d_, int nrows, const StepParams& p_,
                                             i64 wave_id, const BoundedRuleStep& step_, const BoundArgs& ba)
        : step(step_), p(p_), d(d_), n(nrows + 2 * K), hp((i64)p_.h * p_.pitch) {
        // column mask from the global index of the lane's word
        const i64 gw = ba.gword0 + d.col;
        const bool inside = gw >= 0 && gw < ba.gwords, last = gw == ba.gwords - 1;
        em.col_lo = inside ? (last ? ba.tail_lo : ~0u) : 0u;
        em.col_hi = inside ? (last ? ba.tail_hi : ~0u) : 0u;
        // rows of the board in tile coordinates, clamped far outside anything a pass touches (|rows| < 2^30)
        constexpr i64 kFar = (i64)1 << 30;
        const i64 lo64 = -ba.grow0 < -kFar ? -kFar : -ba.grow0;
        const i64 hi64 = ba.grows - ba.grow0 > kFar ? kFar : ba.grows - ba.grow0;
        em.span = (u32)(hi64 - lo64);
        const int a = (int)lo64 - d.row0 + K;
        em.A = MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(a) : a;

        lrow = d.row0 - K;
        if (ROWS == ROWS_WRAP && lrow < 0) lrow += p.h;
        ld = reinterpret_cast<const uint2*>(src + (i64)(lrow + p.R) * p.pitch + (d.col + 1));
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

    template <int PH>
    __device__ __forceinline__ void fetch(u32& lo, u32& hi) {
        uint2 x;
        if constexpr (D == 3) {
            x = pf[PH];
            ROW_LOAD_INTO(pf[PH]);
        } else {
            x = pf[0];
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
        em.apply(lo, hi, i);  // the loaded row: ghost rows and ghost words hold the torus neighbour's cells
        if (!step.template advance<K, PH, GUARD>(P, lo, hi, i, em)) return;
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
        constexpr int i0 = ((2 * K + 2) / 3) * 3;
        int i = 0;
        for (; i < i0; i += 3) {
            body<0, true>(i);
            body<1, true>(i + 1);
            body<2, true>(i + 2);
        }
        if constexpr (D == 6) {
#define BOUNDED_ROW6_STEP(J)                                  \
    compute_store<(J) % 3, false>(pf[J].x, pf[J].y, i + (J)); \
    ROW_LOAD_INTO(pf[J]);                                     \
    next_row();                                               \
    __builtin_amdgcn_sched_barrier(0);
            for (; i + 6 <= n; i += 6) {
                BOUNDED_ROW6_STEP(0) BOUNDED_ROW6_STEP(1) BOUNDED_ROW6_STEP(2) BOUNDED_ROW6_STEP(3) BOUNDED_ROW6_STEP(4)
                BOUNDED_ROW6_STEP(5)
            }
#undef BOUNDED_ROW6_STEP
            if (i < n) compute_store<0, false>(pf[0].x, pf[0].y, i);
            if (i + 1 < n) compute_store<1, false>(pf[1].x, pf[1].y, i + 1);
            if (i + 2 < n) compute_store<2, false>(pf[2].x, pf[2].y, i + 2);
            if (i + 3 < n) compute_store<0, false>(pf[3].x, pf[3].y, i + 3);
            if (i + 4 < n) compute_store<1, false>(pf[4].x, pf[4].y, i + 4);
        } else {
            for (; i + 3 <= n; i += 3) {
                const uint2 x0 = pf[0], x1 = pf[1], x2 = pf[2];
                ROW_LOAD_INTO(pf[0]);
                next_row();
                ROW_LOAD_INTO(pf[1]);
                next_row();
                ROW_LOAD_INTO(pf[2]);
                next_row();
                __builtin_amdgcn_sched_barrier(0);
                // K = 8: a scheduling barrier keeps the third row of a triple apart from the first two.  Left free,
                // the scheduler interleaves the three rows' level chains and the steady loop takes 256 VGPRs plus
                // AGPR copies, 1 wave per SIMD (32768^2: 37.9 us/gen against the torus kernel's 22.7); with the one
                // barrier 184 / 255 VGPRs, 2 waves as step_rule<8> (24.2); a barrier after each of the two rows
                // costs the overlap of the rows' chains (28.7).  docs/PERFORMANCE.md "Bounded boards".
                compute_store<0, false>(x0.x, x0.y, i);
                if constexpr (K >= 8 && (GOL_BOUNDED_ROW_BARRIERS & 1)) __builtin_amdgcn_sched_barrier(0);
                compute_store<1, false>(x1.x, x1.y, i + 1);
                if constexpr (K >= 8 && (GOL_BOUNDED_ROW_BARRIERS & 2)) __builtin_amdgcn_sched_barrier(0);
                compute_store<2, false>(x2.x, x2.y, i + 2);
            }
            if (i < n) body<0, false>(i);
            if (i + 1 < n) body<1, false>(i + 1);
        }
    }
};

template <int K, int ROWS>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_rule_bounded(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                          const LaneDesc* __restrict__ plan, StepParams p,
                                                                          RuleMasks rm, BoundArgs ba) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    // one segment per wave (or packed segments of the same rows): the row masks are scalar
    const bool uni = __builtin_amdgcn_ballot_w64(d.row0 != __builtin_amdgcn_readfirstlane(d.row0)) == 0;
    if (uni) {
        BoundedRunner<K, ROWS, MASK_UNI> w(src, dst, d, nrows, p, wave, BoundedRuleStep(rm), ba);
        w.run();
    } else {
        BoundedRunner<K, ROWS, MASK_LANE> w(src, dst, d, nrows, p, wave, BoundedRuleStep(rm), ba);
        w.run();
    }
}

template <int K>
const void* bounded_kernel_for(u32 flags) {
    return (flags & STEP_WRAP_Y) ? (const void*)step_rule_bounded<K, ROWS_WRAP> : (const void*)step_rule_bounded<K, ROWS_GHOST>;
}

#define FOR_EACH_RULE_DEPTH(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

const void* bounded_kernel_of(int k, u32 flags) {
    switch (k) {
#define DEPTH_CASE(K) \
    case K:           \
        return bounded_kernel_for<K>(flags);
        FOR_EACH_RULE_DEPTH(DEPTH_CASE)
#undef DEPTH_CASE
        default:
            return nullptr;
    }
}

}  // namespace

int rule_bounded_blocks_per_cu(int k, u32 flags) {
    const void* f = bounded_kernel_of(k, flags);
    int nb = 0;
    if (!f || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 64 * kWavesPerBlock, 0) != hipSuccess || nb < 1) return 1;
    return std::min(nb, 32 / kWavesPerBlock);
}

void launch_step_rule_bounded(int k, const Rule& rule, const BoardEdges& edges, const u64* src, u64* dst,
                              const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_rule_bounded has no seam-reading variant (sub-tiles run the torus only)");
    if ((rule.birth & 1u) || rule.birth > 0x1FFu || rule.survive > 0x1FFu)
        throw Error("step_rule_bounded: rule masks outside B1..8 / S0..8 (B0 is out of scope)");
    if (edges.rows < 1 || edges.cols < 1 || edges.row0 < 0 || edges.row0 >= edges.rows || edges.word0 < 0 ||
        edges.word0 >= ceil_div(edges.cols, 64))
        throw Error(strprintf("step_rule_bounded: tile at row %lld, word %lld outside the %lld x %lld board",
                              (long long)edges.row0, (long long)edges.word0, (long long)edges.rows, (long long)edges.cols));
    const void* f = bounded_kernel_of(k, p.flags);
    if (!f) throw Error(strprintf("no bounded rule kernel instantiated for depth %d", k));
    const dim3 grid((unsigned)(n_waves / kWavesPerBlock)), block(64 * kWavesPerBlock);
    StepParams pp = p;
    if (!pp.trash) pp.trash = trash_of_current_device();
    RuleMasks rm{rule.birth, rule.survive};
    const i64 gwords = ceil_div(edges.cols, 64);
    const u64 tail = storage_mask(gwords - 1, edges.cols);
    BoundArgs ba{edges.row0, edges.rows, edges.word0, gwords, (u32)tail, (u32)(tail >> 32)};
    void* args[] = {(void*)&src, (void*)&dst, (void*)&plan, (void*)&pp, (void*)&rm, (void*)&ba};
    hipError_t e = hipLaunchKernel(f, grid, block, args, 0, s);
    if (e != hipSuccess) throw Error(strprintf("bounded rule kernel launch failed: %s", hipGetErrorString(e)));
}

}  // namespace hipk
}  // namespace gol
