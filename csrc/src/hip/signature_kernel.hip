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
// What is step_census's, unchanged (census_kernel.hip): the plans, StepParams, the streaming wave, the rule gates,
// the register ring, the edge masks, the ownership test and the two runners.  The runner and the gates are copied,
// not shared: the other kernels' translation units, and with them their gfx950 code, stay byte for byte what they
// were.  So the kernel reads and writes exactly the rows and words step_temporal<K> does for the same plan, and
// validate_plan covers it.
//
// slots (the slot of the pass's first generation) == nullptr skips the atomics (uniformly): the engine's init-time
// timing launches.
//
// Depths K = 1 .. kMaxSignatureDepth, both row modes, both boundaries; registers: docs/PERFORMANCE.md section 22.
#include "gol/bits.hpp"
#include "gol/hip_kernels.hpp"
#include "gol/signature.hpp"
#include "stencil_device.hpp"
#include "wave_runner.hpp"

// Which rows of a K = 8 row triple a scheduling barrier follows (as GOL_CENSUS_ROW_BARRIERS).
#ifndef GOL_SIGNATURE_ROW_BARRIERS
#define GOL_SIGNATURE_ROW_BARRIERS 2
#endif

namespace gol {
namespace hipk {

namespace {

constexpr int kMaxSignatureDepth = 8;

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

// The tile's place on the board (always), the board's edges (BOUNDED) and the tile's own cells.
struct SigArgs {
    i64 grow0;             // global row of tile row 0
    i64 grows;             // rows of the global board (H)
    i64 gword0;            // global word index of tile word 0
    i64 gwords;            // words per global row, ceil(W / 64)
    u32 tail_lo, tail_hi;  // valid cells of the board's last word, split order
    u32 own_lo, own_hi;    // cells of the tile in its word nw - 1, split order
};

enum { MASK_UNI = 1, MASK_LANE = 2 };  // one row0 per wave (scalar row tests and keys) / row0 per lane

// Edge masks of step_rule_bounded (BOUNDED), the ownership masks and the signature keys of one lane.
template <int MASK, bool BOUNDED>
struct SigMask {
    u32 col_lo, col_hi;  // BOUNDED: in-board cells of the lane's word
    int A;               // BOUNDED: row mask offset
    u32 span;
    u32 own_lo, own_hi;  // counted cells of the lane's word (0 for lanes that own nothing)
    int Ao;              // owned rows: (u32)(t - Ao) < ospan
    u32 ospan;
    u32 gam_e, gam_o;    // column keys of the lane's word
    u32 growb;           // (u32) global row of row counter t = 0: grow0 + row0 - K

    // The key of the global row of row counter t, a value of its own at every use (the header tells why).
    __device__ __forceinline__ u32 row_key(int t) const {
        if (MASK == MASK_UNI) {
            u32 r = sig_rho(growb + (u32)t);
            asm volatile("" : "+s"(r));
            return r;
        }
        asm volatile("" : "+s"(t));
        return sig_rho(growb + (u32)t);
    }

    __device__ __forceinline__ void apply(u32& lo, u32& hi, int t) const {
        if (BOUNDED) {
            const u32 r = (u32)(t - A) < span ? ~0u : 0u;
            lo = b3<kLutAnd3>(lo, col_lo, r);
            hi = b3<kLutAnd3>(hi, col_hi, r);
        }
    }
    // rho: the key of the global row of row counter t
    __device__ __forceinline__ void count(u32& acc, unsigned long long* sig, u32 lo, u32 hi, int t, u32 rho) const {
        const u32 r = (u32)(t - Ao) < ospan ? ~0u : 0u;
        const u32 o = b3<kLutAnd3>(hi, own_hi, r);
        const u32 e = b3<kLutAnd3>(lo, own_lo, r);
        acc = (u32)__builtin_popcount(o) + acc;
        acc = (u32)__builtin_popcount(e) + acc;
        const u64 p = (u64)e * (u64)(rho * gam_e) + (u64)o * (u64)(rho * gam_o);
        atomicAdd(sig, (unsigned long long)p);  // (the lane's own LDS slot: a ds_add_u64 without return)
    }
};

// CensusRuleStep of census_kernel.hip with the per-level signature.
struct SigRuleStep {
    u32 B[9];
    u32 S[9];

    __device__ __forceinline__ explicit SigRuleStep(const RuleMasks& m) {
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

    // CensusRuleStep::advance; the (masked) output of level l is also hashed into sig[l].
    template <int K, int PH, bool GUARD, int MASK, bool BOUNDED>
    __device__ __forceinline__ bool advance(Pipe<K>& P, u32& lo, u32& hi, int i, const SigMask<MASK, BOUNDED>& cm,
                                            u32 (&acc)[K], unsigned long long* sig) const {
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
            const int t = i - (l + 1);
            cm.apply(lo, hi, t);
            cm.count(acc[l], sig + l * (64 * kWavesPerBlock), lo, hi, t, cm.row_key(t));
        }
        return true;
    }
};

// CensusRunner of census_kernel.hip: addresses, next_row, the prefetch and the loops are its, line for line.
template <int K, int ROWS, int MASK, bool BOUNDED>
struct SigRunner {
    static_assert(ROWS == ROWS_GHOST || ROWS == ROWS_WRAP, "step_signature reads ghost rows or wraps");
    static constexpr int D = prefetch_rows<K>();
    const SigRuleStep step;
    const StepParams& p;
    const LaneDesc& d;
    const int n;   // row iterations: nrows + 2K
    const i64 hp;  // h * pitch
    SigMask<MASK, BOUNDED> cm;
    const uint2* ld;
    uint2* st;
    i64 st_stride;
    int lrow;
    uint2 pf[D];
    Pipe<K> P;
    u32 acc[K];
    unsigned long long* sig;  // LDS: level l's accumulator of this lane at sig[l * block size]

    __device__ __forceinline__ void next_row() {
        ld += p.pitch;
        if (ROWS == ROWS_WRAP) {
            ++lrow;
            const bool w = lrow == p.h;
            lrow = w ? 0 : lrow;
            ld = w ? ld - hp : ld;
        }
    }

    __device__ __forceinline__ SigRunner(const u64* src, u64* dst, const LaneDesc& d_, int nrows, const StepParams& p_,
                                         i64 wave_id, const SigRuleStep& step_, const SigArgs& ca, unsigned long long* lds)
        : step(step_), p(p_), d(d_), n(nrows + 2 * K), hp((i64)p_.h * p_.pitch), sig(lds + threadIdx.x) {
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
        // the keys: the lane's two column keys, and the global row of row counter 0
        const u32 gw2 = 2u * (u32)(ca.gword0 + d.col);
        cm.gam_e = sig_gam(gw2);
        cm.gam_o = sig_gam(gw2 + 1u);
        const int gb = (int)(u32)(ca.grow0 + (i64)d.row0 - K);
        cm.growb = (u32)(MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(gb) : gb);
#pragma unroll
        for (int l = 0; l < K; ++l) {
            acc[l] = 0;
            sig[l * (64 * kWavesPerBlock)] = 0;
        }

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
        if (!step.template advance<K, PH, GUARD>(P, lo, hi, i, cm, acc, sig)) return;
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
#define SIG_ROW6_STEP(J)                                      \
    compute_store<(J) % 3, false>(pf[J].x, pf[J].y, i + (J)); \
    ROW_LOAD_INTO(pf[J]);                                     \
    next_row();                                               \
    __builtin_amdgcn_sched_barrier(0);
            for (; i + 6 <= n; i += 6) {
                SIG_ROW6_STEP(0) SIG_ROW6_STEP(1) SIG_ROW6_STEP(2) SIG_ROW6_STEP(3) SIG_ROW6_STEP(4) SIG_ROW6_STEP(5)
            }
#undef SIG_ROW6_STEP
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
                if constexpr (K >= 8 && (GOL_SIGNATURE_ROW_BARRIERS & 1)) __builtin_amdgcn_sched_barrier(0);
                compute_store<1, false>(x1.x, x1.y, i + 1);
                if constexpr (K >= 8 && (GOL_SIGNATURE_ROW_BARRIERS & 2)) __builtin_amdgcn_sched_barrier(0);
                compute_store<2, false>(x2.x, x2.y, i + 2);
            }
            if (i < n) body<0, false>(i);
            if (i + 1 < n) body<1, false>(i + 1);
        }
    }

    // The wave's count and signature of each level: summed over the lanes, two 64-bit atomics per level from lane 0.
    __device__ __forceinline__ void flush(u64* slots, i64 wave_id) const {
        if (!slots) return;
        const size_t stripe = (size_t)(wave_id & (kSigStripes - 1)) * kSigStripeWords;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            u32 v = acc[l];
            const unsigned long long sl = sig[l * (64 * kWavesPerBlock)];
            u32 s_lo = (u32)sl, s_hi = (u32)(sl >> 32);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                v += __shfl_xor(v, off, 64);
                // 64-bit wrapping add over the lanes, in halves with the carry
                const u32 o_lo = __shfl_xor(s_lo, off, 64), o_hi = __shfl_xor(s_hi, off, 64);
                const u32 n_lo = s_lo + o_lo;
                s_hi = s_hi + o_hi + (n_lo < s_lo ? 1u : 0u);
                s_lo = n_lo;
            }
            if ((threadIdx.x & 63) == 0 && v != 0) {
                // (no live owned cell: the signature's share is 0 too)
                u64* slot = slots + (size_t)l * kSigSlotWords + stripe;
                atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)v);
                atomicAdd(reinterpret_cast<unsigned long long*>(slot + kSigSigOffset),
                          ((unsigned long long)s_hi << 32) | (unsigned long long)s_lo);
            }
        }
    }
};

template <int K, int ROWS, bool BOUNDED>
// (the second launch bound: at least two waves per SIMD, so at most 256 registers and none of them an AGPR copy)
__global__ __launch_bounds__(64 * kWavesPerBlock, 2) void step_signature(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                       const LaneDesc* __restrict__ plan, StepParams p,
                                                                       RuleMasks rm, SigArgs ca, u64* __restrict__ slots) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    __shared__ unsigned long long lds[K * 64 * kWavesPerBlock];  // the lanes' signature accumulators (no barrier: each its own)
    // one segment per wave (or packed segments of the same rows): the row tests and the row keys are scalar
    const bool uni = __builtin_amdgcn_ballot_w64(d.row0 != __builtin_amdgcn_readfirstlane(d.row0)) == 0;
    if (uni) {
        SigRunner<K, ROWS, MASK_UNI, BOUNDED> w(src, dst, d, nrows, p, wave, SigRuleStep(rm), ca, lds);
        w.run();
        w.flush(slots, wave);
    } else {
        SigRunner<K, ROWS, MASK_LANE, BOUNDED> w(src, dst, d, nrows, p, wave, SigRuleStep(rm), ca, lds);
        w.run();
        w.flush(slots, wave);
    }
}

template <int K>
const void* signature_kernel_for(u32 flags, bool bounded) {
    if (bounded)
        return (flags & STEP_WRAP_Y) ? (const void*)step_signature<K, ROWS_WRAP, true> : (const void*)step_signature<K, ROWS_GHOST, true>;
    return (flags & STEP_WRAP_Y) ? (const void*)step_signature<K, ROWS_WRAP, false> : (const void*)step_signature<K, ROWS_GHOST, false>;
}

#define FOR_EACH_SIGNATURE_DEPTH(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

const void* signature_kernel_of(int k, u32 flags, bool bounded) {
    switch (k) {
#define DEPTH_CASE(K) \
    case K:           \
        return signature_kernel_for<K>(flags, bounded);
        FOR_EACH_SIGNATURE_DEPTH(DEPTH_CASE)
#undef DEPTH_CASE
        default:
            return nullptr;
    }
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

int max_signature_depth() { return kMaxSignatureDepth; }

int signature_blocks_per_cu(int k, u32 flags, bool bounded) {
    const void* f = signature_kernel_of(k, flags, bounded);
    int nb = 0;
    if (!f || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 64 * kWavesPerBlock, 0) != hipSuccess || nb < 1) return 1;
    return std::min(nb, 32 / kWavesPerBlock);
}

void launch_step_signature(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src,
                           u64* dst, const LaneDesc* plan, i64 n_waves, const StepParams& p, u64* slots, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_signature has no seam-reading variant (sub-tiles do not run signature mode)");
    if ((rule.birth & 1u) || rule.birth > 0x1FFu || rule.survive > 0x1FFu)
        throw Error("step_signature: rule masks outside B1..8 / S0..8 (B0 is out of scope)");
    if (place.rows < 1 || place.cols < 1 || place.row0 < 0 || place.row0 >= place.rows || place.word0 < 0 ||
        place.word0 >= ceil_div(place.cols, 64))
        throw Error(strprintf("step_signature: tile at row %lld, word %lld outside the %lld x %lld board", (long long)place.row0,
                              (long long)place.word0, (long long)place.rows, (long long)place.cols));
    if (tile_cols < 1 || ceil_div(tile_cols, 64) != (i64)p.nw)
        throw Error(strprintf("step_signature: a tile of %lld columns does not have %d words", (long long)tile_cols, (int)p.nw));
    const void* f = signature_kernel_of(k, p.flags, bounded);
    if (!f) throw Error(strprintf("no signature kernel instantiated for depth %d (1..%d)", k, kMaxSignatureDepth));
    const dim3 grid((unsigned)(n_waves / kWavesPerBlock)), block(64 * kWavesPerBlock);
    StepParams pp = p;
    if (!pp.trash) pp.trash = trash_of_current_device();
    RuleMasks rm{rule.birth, rule.survive};
    const i64 gwords = ceil_div(place.cols, 64);
    const u64 tail = storage_mask(gwords - 1, place.cols);
    const u64 own = storage_mask((i64)p.nw - 1, tile_cols);
    SigArgs ca{place.row0, place.rows, place.word0, gwords, (u32)tail, (u32)(tail >> 32), (u32)own, (u32)(own >> 32)};
    void* args[] = {(void*)&src, (void*)&dst, (void*)&plan, (void*)&pp, (void*)&rm, (void*)&ca, (void*)&slots};
    hipError_t e = hipLaunchKernel(f, grid, block, args, 0, s);
    if (e != hipSuccess) throw Error(strprintf("signature kernel launch failed: %s", hipGetErrorString(e)));
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
