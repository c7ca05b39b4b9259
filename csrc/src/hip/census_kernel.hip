// gol-mi355x: step_census<K, ROWS, BOUNDED> -- step_rule / step_rule_bounded that also counts the live cells of
// every generation it computes, for gfx950 (CDNA4).
//
// A temporal-blocked pass keeps generations 1 .. K - 1 in registers only, so the population of each generation can
// be counted nowhere but here.  Each level's output is already in two VGPRs (the word's even and odd cells); the
// count is a masked v_bcnt_u32_b32 of each into one accumulator per level:
//     acc[l] = bcnt(lo & own_lo & own_row, bcnt(hi & own_hi & own_row, acc[l]))      (2 v_bitop3 + 2 v_bcnt)
// and at the end of the wave each acc[l] is summed over the lanes and one lane adds it to the slot of level l with
// one 64-bit atomic: K atomics per wave, no other memory traffic.  A generation's slot is kCensusStripes partial
// sums, each on a 128-byte line of its own (the host adds them up); a wave adds into stripe  wave id mod
// kCensusStripes.  Atomics on one cache line complete one after the other, about 12-16 ns each, and the waves of a
// one-round plan all end together: with the K slots of a pass packed into one line the 8600 atomics of an 8192^2
// pass took longer than the pass computes (17.2 us/gen against step_rule's 4.5), with one line per generation 6.6
// (docs/PERFORMANCE.md section 21).
//
// What is step_rule_bounded's, unchanged (rule_bounded_kernel.hip): the plans, StepParams, the streaming wave (the
// load stream, the prefetch depth, ROWS_GHOST / ROWS_WRAP, one store per row from row 2K on, the trash slots), the
// rule gates, the register ring, the edge masks and the two runners (scalar row tests for a wave of one row0,
// per-lane tests for packed narrow segments).  The runner and the gates are copied, not shared: the other
// kernels' translation units, and with them their gfx950 code, stay byte for byte what they were.  So the kernel
// reads and writes exactly the rows and words step_temporal<K> does for the same plan, and validate_plan covers it.
//
// BOUNDED is a template parameter: on the torus the edge masks (two and3 per level, the column masks' two VGPRs
// and the loaded row's mask) are compiled out, so the torus census keeps step_rule's values in every word it
// stores (the tail bits of an unaligned last word included) and a few registers more free than a kernel handed
// "everything is inside" masks would.
//
// Ownership.  A pass computes many cells more than once: the halo lanes, the 2K extra rows of every segment, the
// extension rows -e .. h + e of the earlier passes of a multi-pass superstep, the ghost words those passes store
// in the 2-D layout.  A cell of the level-j output (j = 1 .. K) of row iteration i, the unwrapped tile row
//     t = row0 - K + i - j                       (the row counter of the bounded kernel's row mask)
// is counted iff the lane stores (LANE_STORE), its word is a word of the tile (0 <= col < nw), the bit is a cell
// of the tile (the tile's storage mask on word nw - 1) and  max(row0, 0) <= t < min(row0 + nrows, h).  The store
// lanes of the segments partition a pass's output region and the regions of a pass (full, or interior and bands)
// partition the tile plus its extension, so every cell of the tile is counted once per level.  A level output
// skipped while the pipeline fills is never an owned row (i >= K + j there, and K + j >= 2 j).
// The row test is  (u32)(i - j - Ao) < ospan  with  Ao = max(row0, 0) - row0 + K: scalar in the UNI runner.
//
// counts (the slot of the pass's first generation) == nullptr skips the atomics (uniformly): the engine's init-time
// timing launches.
//
// Depths K = 1 .. kMaxCensusDepth, both row modes, both boundaries; registers: docs/PERFORMANCE.md section 21.
#include "gol/bits.hpp"
#include "gol/hip_kernels.hpp"
#include "stencil_device.hpp"
#include "wave_runner.hpp"

// Which rows of a K = 8 row triple a scheduling barrier follows (as GOL_BOUNDED_ROW_BARRIERS).
#ifndef GOL_CENSUS_ROW_BARRIERS
#define GOL_CENSUS_ROW_BARRIERS 2
#endif

namespace gol {
namespace hipk {

namespace {

constexpr int kMaxCensusDepth = 8;

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

// The board's edges (as step_rule_bounded's BoundArgs; unused on the torus) and the tile's own cells.
struct CensusArgs {
    i64 grow0;             // global row of tile row 0
    i64 grows;             // rows of the global board (H)
    i64 gword0;            // global word index of tile word 0
    i64 gwords;            // words per global row, ceil(W / 64)
    u32 tail_lo, tail_hi;  // valid cells of the board's last word, split order
    u32 own_lo, own_hi;    // cells of the tile in its word nw - 1, split order
};

enum { MASK_UNI = 1, MASK_LANE = 2 };  // one row0 per wave (scalar row tests) / row0 per lane

// Edge masks of step_rule_bounded (BOUNDED) and the ownership masks of one lane.
template <int MASK, bool BOUNDED>
struct CensusMask {
    u32 col_lo, col_hi;  // BOUNDED: in-board cells of the lane's word
    int A;               // BOUNDED: row mask offset
    u32 span;
    u32 own_lo, own_hi;  // counted cells of the lane's word (0 for lanes that own nothing)
    int Ao;              // owned rows: (u32)(t - Ao) < ospan
    u32 ospan;

    __device__ __forceinline__ void apply(u32& lo, u32& hi, int t) const {
        if (BOUNDED) {
            const u32 r = (u32)(t - A) < span ? ~0u : 0u;
            lo = b3<kLutAnd3>(lo, col_lo, r);
            hi = b3<kLutAnd3>(hi, col_hi, r);
        }
    }
    __device__ __forceinline__ void count(u32& acc, u32 lo, u32 hi, int t) const {
        const u32 r = (u32)(t - Ao) < ospan ? ~0u : 0u;
        acc = (u32)__builtin_popcount(b3<kLutAnd3>(hi, own_hi, r)) + acc;
        acc = (u32)__builtin_popcount(b3<kLutAnd3>(lo, own_lo, r)) + acc;
    }
};

// BoundedRuleStep of rule_bounded_kernel.hip with the per-level count.
struct CensusRuleStep {
    u32 B[9];
    u32 S[9];

    __device__ __forceinline__ explicit CensusRuleStep(const RuleMasks& m) {
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

    // BoundedRuleStep::advance; the (masked) output of level l is counted into acc[l].
    template <int K, int PH, bool GUARD, int MASK, bool BOUNDED>
    __device__ __forceinline__ bool advance(Pipe<K>& P, u32& lo, u32& hi, int i, const CensusMask<MASK, BOUNDED>& cm,
                                            u32 (&acc)[K]) const {
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
            cm.apply(lo, hi, i - (l + 1));
            cm.count(acc[l], lo, hi, i - (l + 1));
        }
        return true;
    }
};

// BoundedRunner of rule_bounded_kernel.hip: addresses, next_row, the prefetch and the loops are its, line for line.
template <int K, int ROWS, int MASK, bool BOUNDED>
struct CensusRunner {
    static_assert(ROWS == ROWS_GHOST || ROWS == ROWS_WRAP, "step_census reads ghost rows or wraps");
    static constexpr int D = prefetch_rows<K>();
    const CensusRuleStep step;
    const StepParams& p;
    const LaneDesc& d;
    const int n;   // row iterations: nrows + 2K
    const i64 hp;  // h * pitch
    CensusMask<MASK, BOUNDED> cm;
    const uint2* ld;
    uint2* st;
    i64 st_stride;
    int lrow;
    uint2 pf[D];
    Pipe<K> P;
    u32 acc[K];

    __device__ __forceinline__ void next_row() {
        ld += p.pitch;
        if (ROWS == ROWS_WRAP) {
            ++lrow;
            const bool w = lrow == p.h;
            lrow = w ? 0 : lrow;
            ld = w ? ld - hp : ld;
        }
    }

    __device__ __forceinline__ CensusRunner(const u64* src, u64* dst, const LaneDesc& d_, int nrows, const StepParams& p_,
                                            i64 wave_id, const CensusRuleStep& step_, const CensusArgs& ca)
        : step(step_), p(p_), d(d_), n(nrows + 2 * K), hp((i64)p_.h * p_.pitch) {
        const bool out = d.flags & LANE_STORE;
        if (BOUNDED) {
            // column mask from the global index of the lane's word
            const i64 gw = ca.gword0 + d.col;
            const bool inside = gw >= 0 && gw < ca.gwords, last = gw == ca.gwords - 1;
            cm.col_lo = inside ? (last ? ca.tail_lo : ~0u) : 0u;
            cm.col_hi = inside ? (last ? ca.tail_hi : ~0u) : 0u;
            // rows of the board in tile coordinates, clamped far outside anything a pass touches (|rows| < 2^30)
            constexpr i64 kFar = (i64)1 << 30;
            const i64 lo64 = -ca.grow0 < -kFar ? -kFar : -ca.grow0;
            const i64 hi64 = ca.grows - ca.grow0 > kFar ? kFar : ca.grows - ca.grow0;
            cm.span = (u32)(hi64 - lo64);
            const int a = (int)lo64 - d.row0 + K;
            cm.A = MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(a) : a;
        }
        // the cells this lane counts: a store lane's word of the tile, rows of the segment inside the tile
        const bool owns = out && d.col >= 0 && d.col < p.nw, tail = d.col == p.nw - 1;
        cm.own_lo = owns ? (tail ? ca.own_lo : ~0u) : 0u;
        cm.own_hi = owns ? (tail ? ca.own_hi : ~0u) : 0u;
        const int olo = d.row0 > 0 ? d.row0 : 0;
        const int ohi = d.row0 + nrows < p.h ? d.row0 + nrows : p.h;
        const int ao = olo - d.row0 + K;
        const u32 os = ohi > olo ? (u32)(ohi - olo) : 0u;
        cm.Ao = MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(ao) : ao;
        cm.ospan = MASK == MASK_UNI ? (u32)__builtin_amdgcn_readfirstlane((int)os) : os;
#pragma unroll
        for (int l = 0; l < K; ++l) acc[l] = 0;

        lrow = d.row0 - K;
        if (ROWS == ROWS_WRAP && lrow < 0) lrow += p.h;
        ld = reinterpret_cast<const uint2*>(src + (i64)(lrow + p.R) * p.pitch + (d.col + 1));
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
        cm.apply(lo, hi, i);  // (BOUNDED) the loaded row: ghost rows and words hold the torus neighbour's cells
        if (!step.template advance<K, PH, GUARD>(P, lo, hi, i, cm, acc)) return;
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
#define CENSUS_ROW6_STEP(J)                                   \
    compute_store<(J) % 3, false>(pf[J].x, pf[J].y, i + (J)); \
    ROW_LOAD_INTO(pf[J]);                                     \
    next_row();                                               \
    __builtin_amdgcn_sched_barrier(0);
            for (; i + 6 <= n; i += 6) {
                CENSUS_ROW6_STEP(0) CENSUS_ROW6_STEP(1) CENSUS_ROW6_STEP(2) CENSUS_ROW6_STEP(3) CENSUS_ROW6_STEP(4)
                CENSUS_ROW6_STEP(5)
            }
#undef CENSUS_ROW6_STEP
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
                // K = 8: the bounded kernel's scheduling barrier, which keeps the third row of a triple apart from
                // the first two (rule_bounded_kernel.hip tells what the steady loop takes without it)
                compute_store<0, false>(x0.x, x0.y, i);
                if constexpr (K >= 8 && (GOL_CENSUS_ROW_BARRIERS & 1)) __builtin_amdgcn_sched_barrier(0);
                compute_store<1, false>(x1.x, x1.y, i + 1);
                if constexpr (K >= 8 && (GOL_CENSUS_ROW_BARRIERS & 2)) __builtin_amdgcn_sched_barrier(0);
                compute_store<2, false>(x2.x, x2.y, i + 2);
            }
            if (i < n) body<0, false>(i);
            if (i + 1 < n) body<1, false>(i + 1);
        }
    }

    // The wave's count of each level: summed over the lanes, one 64-bit atomic per level from lane 0.
    __device__ __forceinline__ void flush(u64* counts, i64 wave_id) const {
        if (!counts) return;
        const size_t stripe = (size_t)(wave_id & (kCensusStripes - 1)) * kCensusStripeWords;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            u32 v = acc[l];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((threadIdx.x & 63) == 0 && v != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(counts + (size_t)l * kCensusSlotWords + stripe), (unsigned long long)v);
        }
    }
};

template <int K, int ROWS, bool BOUNDED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_census(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                    const LaneDesc* __restrict__ plan, StepParams p,
                                                                    RuleMasks rm, CensusArgs ca, u64* __restrict__ counts) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    // one segment per wave (or packed segments of the same rows): the row tests are scalar
    const bool uni = __builtin_amdgcn_ballot_w64(d.row0 != __builtin_amdgcn_readfirstlane(d.row0)) == 0;
    if (uni) {
        CensusRunner<K, ROWS, MASK_UNI, BOUNDED> w(src, dst, d, nrows, p, wave, CensusRuleStep(rm), ca);
        w.run();
        w.flush(counts, wave);
    } else {
        CensusRunner<K, ROWS, MASK_LANE, BOUNDED> w(src, dst, d, nrows, p, wave, CensusRuleStep(rm), ca);
        w.run();
        w.flush(counts, wave);
    }
}

template <int K>
const void* census_kernel_for(u32 flags, bool bounded) {
    if (bounded)
        return (flags & STEP_WRAP_Y) ? (const void*)step_census<K, ROWS_WRAP, true> : (const void*)step_census<K, ROWS_GHOST, true>;
    return (flags & STEP_WRAP_Y) ? (const void*)step_census<K, ROWS_WRAP, false> : (const void*)step_census<K, ROWS_GHOST, false>;
}

#define FOR_EACH_CENSUS_DEPTH(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

const void* census_kernel_of(int k, u32 flags, bool bounded) {
    switch (k) {
#define DEPTH_CASE(K) \
    case K:           \
        return census_kernel_for<K>(flags, bounded);
        FOR_EACH_CENSUS_DEPTH(DEPTH_CASE)
#undef DEPTH_CASE
        default:
            return nullptr;
    }
}

}  // namespace

int max_census_depth() { return kMaxCensusDepth; }

int census_blocks_per_cu(int k, u32 flags, bool bounded) {
    const void* f = census_kernel_of(k, flags, bounded);
    int nb = 0;
    if (!f || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 64 * kWavesPerBlock, 0) != hipSuccess || nb < 1) return 1;
    return std::min(nb, 32 / kWavesPerBlock);
}

void launch_step_census(int k, const Rule& rule, const BoardEdges* edges, i64 tile_cols, const u64* src, u64* dst,
                        const LaneDesc* plan, i64 n_waves, const StepParams& p, u64* counts, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_census has no seam-reading variant (sub-tiles do not run the census)");
    if ((rule.birth & 1u) || rule.birth > 0x1FFu || rule.survive > 0x1FFu)
        throw Error("step_census: rule masks outside B1..8 / S0..8 (B0 is out of scope)");
    if (edges && (edges->rows < 1 || edges->cols < 1 || edges->row0 < 0 || edges->row0 >= edges->rows || edges->word0 < 0 ||
                  edges->word0 >= ceil_div(edges->cols, 64)))
        throw Error(strprintf("step_census: tile at row %lld, word %lld outside the %lld x %lld board", (long long)edges->row0,
                              (long long)edges->word0, (long long)edges->rows, (long long)edges->cols));
    if (tile_cols < 1 || ceil_div(tile_cols, 64) != (i64)p.nw)
        throw Error(strprintf("step_census: a tile of %lld columns does not have %d words", (long long)tile_cols, (int)p.nw));
    const void* f = census_kernel_of(k, p.flags, edges != nullptr);
    if (!f) throw Error(strprintf("no census kernel instantiated for depth %d (1..%d)", k, kMaxCensusDepth));
    const dim3 grid((unsigned)(n_waves / kWavesPerBlock)), block(64 * kWavesPerBlock);
    StepParams pp = p;
    if (!pp.trash) pp.trash = trash_of_current_device();
    RuleMasks rm{rule.birth, rule.survive};
    CensusArgs ca{};
    if (edges) {
        const i64 gwords = ceil_div(edges->cols, 64);
        const u64 tail = storage_mask(gwords - 1, edges->cols);
        ca = CensusArgs{edges->row0, edges->rows, edges->word0, gwords, (u32)tail, (u32)(tail >> 32), 0, 0};
    }
    const u64 own = storage_mask((i64)p.nw - 1, tile_cols);
    ca.own_lo = (u32)own;
    ca.own_hi = (u32)(own >> 32);
    void* args[] = {(void*)&src, (void*)&dst, (void*)&plan, (void*)&pp, (void*)&rm, (void*)&ca, (void*)&counts};
    hipError_t e = hipLaunchKernel(f, grid, block, args, 0, s);
    if (e != hipSuccess) throw Error(strprintf("census kernel launch failed: %s", hipGetErrorString(e)));
}

}  // namespace hipk
}  // namespace gol
