// gol-mi355x: step_ltl<R, BOUNDED, MASK> -- one generation of a Larger than Life rule (gol/rule.hpp: two states, the
// box of range R = 1 .. 7, birth and survival by count intervals) per pass, for gfx950 (CDNA4).
//
// The wave is the streaming wave of the other kernels: LaneDesc plans (62 output + 2 halo lanes, one word column per
// lane), StepParams, rows read modulo h (ROWS_WRAP: the engine runs these rules on one rank), split words, a trash slot
// for the lanes that store nothing.  A generation of range R has the dependency cone of R Life generations, so the
// plan is that of a pass of depth R and the load stream is WaveRunner<R, ROWS_WRAP>'s: it begins at row row0 - R,
// runs over n = nrows + 2R rows and stores one row per input row from row 2R on.
//
// INVARIANT (rule_runner.hpp states it for the generic kernels): for the same plan and StepParams this kernel reads and
// writes no row or word step_temporal<R> would not.  It writes the same words.  It reads fewer: the prefetch stops at
// the segment's last input row (the load of row i + kAhead is skipped when that row is not one of the n), so nothing
// is read past it, where step_temporal<R> reads 3 or 6 rows into the slack.  validate_plan(..., k = R, ...) is
// therefore the whole host-side safety check.
//
// Per row and word half:
//   * horizontal: the 2R + 1 cells of the window as shifted copies of the two halves.  In the split format an even
//     cell's window is lo at bit offsets -floor(R/2) .. floor(R/2) and hi at -ceil(R/2) .. ceil(R/2) - 1; the odd half
//     is the mirror image (hi at -floor .. floor, lo at -ceil + 1 .. ceil).  Offsets are at most 4 bits, so each half
//     takes one dpp_prev and one dpp_next and one v_alignbit_b32 per shifted copy (2R per row, shared by the halves).
//     The copies are added by a column compression of full adders (xor3 / maj, v_bitop3_b32) into kHP = bit_width(2R+1)
//     planes: 2, 3, 3, 4, 4, 4, 4.
//   * vertical: a running column sum T over the last 2R + 1 rows, centre cell included, in kP = bit_width((2R+1)^2)
//     planes (4, 5, 6, 7, 7, 8, 8): the leaving row's horizontal sum is subtracted and the entering row's added, two
//     ripple chains of two gates per plane.  The leaving sum comes from a register ring of the 2R + 1 horizontal sums,
//     (2R+1) x kHP x 2 registers, up to 120 at R = 7.  The other way, a ring of the raw rows (30 registers) whose
//     leaving sum is formed again, costs the horizontal stage twice (about 70 more VALU per row at R = 7) in a kernel
//     that is VALU-bound; the sums' ring fits without scratch or AGPRs at every R (docs/PERFORMANCE.md section 32 has
//     the counts), so it was built.  The ring's slot is the row's phase, so the row loop is unrolled 2R + 1 times; it
//     starts at zero, and the fill phase subtracts zeros instead of branching.
//   * rule: the host folds M into four thresholds on T (Rule::ltl_thresholds); each is compared bit-sliced, one
//     v_bitop3 per plane, against a constant whose bits are uniform all-ones or all-zeros words (one SGPR operand per
//     instruction, all a VOP3 of this ISA reads; rule_runner.hpp), then a mux on the centre cell, which a ring of raw
//     rows keeps for R rows.
//   * bounded boards: EdgeMask<MASK> (rule_runner.hpp) on the loaded row and on the output, as step_rule_bounded;
//     MASK_UNI or MASK_LANE is chosen per wave by one_row0.
// No scratch, no AGPRs, no LDS, no atomics, plain vector stores.
#include "rule_launch.hpp"

namespace gol {
namespace hipk {

namespace {

// The rule's four thresholds on T (Rule::ltl_thresholds): run-time, wave-uniform, a kernel argument of their own.
struct LtlArgs {
    u32 blo, bhi, slo, shi;
};

constexpr int bit_width_of(int v) { return v == 0 ? 0 : 1 + bit_width_of(v >> 1); }
constexpr int ltl_hplanes(int R) { return bit_width_of(2 * R + 1); }
constexpr int ltl_planes(int R) { return bit_width_of((2 * R + 1) * (2 * R + 1)); }
// Rows loaded ahead.  The slot of a prefetched row is its phase modulo this, so it divides 2R + 1; no row past the
// segment's last input row is loaded whatever it is (LtlRunner::row).
constexpr int ltl_ahead(int R) { return R == 4 ? 3 : (R == 7 ? 5 : 2 * R + 1); }

constexpr unsigned kLutBorrow = lut3([](unsigned t, unsigned h, unsigned b) { return (~t & (h | b)) | (h & b); });
constexpr unsigned kLutAndNot = lut3([](unsigned a, unsigned b, unsigned) { return ~a & b; });
// one plane of T >= c and of T <= c, from the least significant plane up: (t, c, so far)
constexpr unsigned kLutGe = lut3([](unsigned t, unsigned c, unsigned g) { return (t & ~c) | (~(t ^ c) & g); });
constexpr unsigned kLutLe = lut3([](unsigned t, unsigned c, unsigned g) { return (~t & c) | (~(t ^ c) & g); });

// x seen s bits along: bit j of the result is bit j + s of x, the bits beyond the word from the neighbouring lanes'
// words (prev: lane - 1, next: lane + 1); |s| <= 31.
__device__ __forceinline__ u32 shifted(u32 x, u32 prev, u32 next, int s) {
    if (s == 0) return x;
    return s > 0 ? __builtin_amdgcn_alignbit(next, x, (u32)s) : __builtin_amdgcn_alignbit(x, prev, (u32)(32 + s));
}

// The sum of N one-bit words of one weight as bit planes out[0 .. bit_width(N)): a chain of full adders through the
// column, the carries summed the same way one weight up.  N - bit_width(N) adders in all when N is 2^k - 1.
template <int N>
struct BitSum {
    static __device__ __forceinline__ void run(const u32* in, u32* out) {
        u32 carry[N / 2 > 0 ? N / 2 : 1];
        u32 s = in[0];
#pragma unroll
        for (int i = 1; i + 1 < N; i += 2) {
            carry[(i - 1) / 2] = b3<kLutMaj>(s, in[i], in[i + 1]);
            s = b3<kLutXor3>(s, in[i], in[i + 1]);
        }
        if constexpr (N % 2 == 0) {  // one word left: a half adder
            carry[N / 2 - 1] = s & in[N - 1];
            s ^= in[N - 1];
        }
        out[0] = s;
        if constexpr (N / 2 > 0) BitSum<N / 2>::run(carry, out + 1);
    }
};

// T += h and T -= h for a T of P planes and an h of HP <= P planes (no overflow and no underflow: the callers' T is a
// sum that holds, or has room for, h).
template <int P, int HP>
__device__ __forceinline__ void planes_add(u32* T, const u32* h) {
    u32 c = T[0] & h[0];
    T[0] ^= h[0];
#pragma unroll
    for (int p = 1; p < P; ++p) {
        if (p < HP) {
            const u32 t = b3<kLutXor3>(T[p], h[p], c);
            c = b3<kLutMaj>(T[p], h[p], c);
            T[p] = t;
        } else {
            const u32 t = T[p] ^ c;
            c = T[p] & c;
            T[p] = t;
        }
    }
}
template <int P, int HP>
__device__ __forceinline__ void planes_sub(u32* T, const u32* h) {
    u32 b = b3<kLutAndNot>(T[0], h[0], h[0]);
    T[0] ^= h[0];
#pragma unroll
    for (int p = 1; p < P; ++p) {
        if (p < HP) {
            const u32 t = b3<kLutXor3>(T[p], h[p], b);
            b = b3<kLutBorrow>(T[p], h[p], b);
            T[p] = t;
        } else {
            const u32 t = T[p] ^ b;
            b = b3<kLutAndNot>(T[p], b, b);
            T[p] = t;
        }
    }
}

// The rule's thresholds as uniform words: bit p of a threshold as all ones or all zeros.
template <int P>
struct LtlGates {
    u32 blo[P], bhi[P], slo[P], shi[P];

    __device__ __forceinline__ explicit LtlGates(const LtlArgs& a) {
#pragma unroll
        for (int p = 0; p < P; ++p) {
            blo[p] = 0u - ((a.blo >> p) & 1u);
            bhi[p] = 0u - ((a.bhi >> p) & 1u);
            slo[p] = 0u - ((a.slo >> p) & 1u);
            shi[p] = 0u - ((a.shi >> p) & 1u);
        }
    }

    // next state of 32 cells from the planes of T (centre included) and the centre cells x
    __device__ __forceinline__ u32 rule(const u32* T, u32 x) const {
        u32 gb = ~0u, lb = ~0u, gs = ~0u, ls = ~0u;
#pragma unroll
        for (int p = 0; p < P; ++p) {
            gb = b3<kLutGe>(T[p], blo[p], gb);
            lb = b3<kLutLe>(T[p], bhi[p], lb);
            gs = b3<kLutGe>(T[p], slo[p], gs);
            ls = b3<kLutLe>(T[p], shi[p], ls);
        }
        const u32 born = b3<kLutAnd2>(gb, lb, lb);
        return b3<kLutMux>(x, gs & ls, born);
    }
};

struct NoEdgeMask {};

// MASK: 0 the torus (no mask), MASK_UNI / MASK_LANE a bounded board (rule_runner.hpp).
template <int R, int MASK>
struct LtlRunner {
    static constexpr int N = 2 * R + 1, HP = ltl_hplanes(R), P = ltl_planes(R), AHEAD = ltl_ahead(R);
    static constexpr int F = R / 2, C = (R + 1) / 2;  // floor(R / 2), ceil(R / 2)
    static_assert(N % AHEAD == 0, "a prefetched row's slot is its phase");
    const LtlGates<P> gates;
    const StepParams& p;
    const int n;   // row iterations: nrows + 2R
    const i64 hp;  // h * pitch
    std::conditional_t<MASK != 0, EdgeMask<MASK != 0 ? MASK : MASK_UNI>, NoEdgeMask> em;
    const uint2* ld;
    uint2* st;
    i64 st_stride;  // pitch for output lanes, 0 for halo/idle lanes (they write a trash slot)
    int lrow;       // tile row of the next load (wave-uniform)
    uint2 pf[AHEAD];
    u32 H[N][2][HP];  // the ring of horizontal sums: slot = the row's phase
    u32 X[N][2];      // the raw rows (the centre cells of the output R rows later)
    u32 T[2][P];      // the column sum over the last N rows, centre included

    __device__ __forceinline__ void next_row() {  // (WaveRunner's, ROWS_WRAP)
        ld += p.pitch;
        ++lrow;
        const bool w = lrow == p.h;
        lrow = w ? 0 : lrow;
        ld = w ? ld - hp : ld;
    }

    __device__ __forceinline__ LtlRunner(const u64* src, u64* dst, const LaneDesc& d, int nrows, const StepParams& p_,
                                         i64 wave_id, const LtlArgs& la, const TileArgs& ta)
        : gates(la), p(p_), n(nrows + 2 * R), hp((i64)p_.h * p_.pitch) {
        if constexpr (MASK != 0) em.template init<R>(d, ta);
        lrow = d.row0 - R;
        if (lrow < 0) lrow += p.h;
        ld = reinterpret_cast<const uint2*>(src + (i64)(lrow + p.R) * p.pitch + (d.col + 1));
        const bool out = d.flags & LANE_STORE;
        st = out ? reinterpret_cast<uint2*>(dst + (i64)(d.row0 + p.R) * p.pitch + (d.col + 1))
                 : reinterpret_cast<uint2*>(p.trash + ((i64)(wave_id & (kTrashWaves - 1)) * 64 + (threadIdx.x & 63)));
        st_stride = out ? p.pitch : 0;
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) {  // (n >= 2R + 1 >= AHEAD: these are input rows)
            ROW_LOAD_INTO(pf[j]);
            next_row();
        }
#pragma unroll
        for (int s = 0; s < N; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int q = 0; q < HP; ++q) H[s][h][q] = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < P; ++q) T[h][q] = 0;
    }

    // The window sums of one row: e[] the even cells' (the lo half), o[] the odd cells'.
    __device__ __forceinline__ void hsum(u32 lo, u32 hi, u32* e, u32* o) const {
        const u32 pl = dpp_prev(lo), nl = dpp_next(lo), ph = dpp_prev(hi), nh = dpp_next(hi);
        // lo and hi seen s bits along, at index s + C: the two windows take lo at -F .. C and hi at -C .. F
        u32 ls[2 * C + 1], hs[2 * C + 1];
#pragma unroll
        for (int s = -C; s <= C; ++s) {
            if (s >= -F) ls[s + C] = shifted(lo, pl, nl, s);
            if (s <= F) hs[s + C] = shifted(hi, ph, nh, s);
        }
        u32 in[N];
        int k = 0;
#pragma unroll
        for (int s = -F; s <= F; ++s) in[k++] = ls[s + C];
#pragma unroll
        for (int s = -C; s <= C - 1; ++s) in[k++] = hs[s + C];
        BitSum<N>::run(in, e);
        k = 0;
#pragma unroll
        for (int s = -F; s <= F; ++s) in[k++] = hs[s + C];
#pragma unroll
        for (int s = -C + 1; s <= C; ++s) in[k++] = ls[s + C];
        BitSum<N>::run(in, o);
    }

    // Row iteration i, of phase PH = i mod N.
    template <int PH>
    __device__ __forceinline__ void row(int i) {
        const uint2 x = pf[PH % AHEAD];
        if (i + AHEAD < n) {  // (uniform) the load stream ends at the segment's last input row
            ROW_LOAD_INTO(pf[PH % AHEAD]);
            next_row();
        }
        u32 lo = x.x, hi = x.y;
        if constexpr (MASK != 0) em.apply(lo, hi, i);
        u32 sum[2][HP];
        hsum(lo, hi, sum[0], sum[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            planes_sub<P, HP>(T[h], H[PH][h]);  // the row that leaves the window (zeros while it fills)
            planes_add<P, HP>(T[h], sum[h]);
#pragma unroll
            for (int q = 0; q < HP; ++q) H[PH][h][q] = sum[h][q];
        }
        X[PH][0] = lo;
        X[PH][1] = hi;
        if (i < 2 * R) return;  // (uniform) the window is not full yet
        constexpr int CEN = (PH + N - R) % N;  // the centre row arrived R rows ago
        u32 olo = gates.rule(T[0], X[CEN][0]);
        u32 ohi = gates.rule(T[1], X[CEN][1]);
        if constexpr (MASK != 0) em.apply(olo, ohi, i - R);
        *st = make_uint2(olo, ohi);
        st += st_stride;
    }

    template <int PH>
    __device__ __forceinline__ bool rows_from(int i) {
        if (i >= n) return false;
        row<PH>(i);
        if constexpr (PH + 1 < N)
            return rows_from<PH + 1>(i + 1);
        else
            return true;
    }

    __device__ __forceinline__ void run() {
        for (int i = 0; rows_from<0>(i); i += N) {
        }
    }
};

// MASK = 0 on a bounded board: the kernel the engine launches, which picks the runner per wave.  The single-runner
// kernels (MASK_UNI, MASK_LANE) are built with GOL_LTL_SPLIT_MASKS for the resource table of docs/PERFORMANCE.md only.
template <int R, bool BOUNDED, int MASK>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_ltl(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                 const LaneDesc* __restrict__ plan, StepParams p, LtlArgs la,
                                                                 TileArgs ta) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if constexpr (!BOUNDED) {
        LtlRunner<R, 0> w(src, dst, d, nrows, p, wave, la, ta);
        w.run();
    } else if constexpr (MASK != 0) {
        LtlRunner<R, MASK> w(src, dst, d, nrows, p, wave, la, ta);
        w.run();
    } else if (one_row0(d)) {
        LtlRunner<R, MASK_UNI> w(src, dst, d, nrows, p, wave, la, ta);
        w.run();
    } else {
        LtlRunner<R, MASK_LANE> w(src, dst, d, nrows, p, wave, la, ta);
        w.run();
    }
}

#ifdef GOL_LTL_SPLIT_MASKS
#define LTL_SPLIT(R)                                            \
    template __global__ void step_ltl<R, true, MASK_UNI>(const u64*, u64*, const LaneDesc*, StepParams, LtlArgs, TileArgs); \
    template __global__ void step_ltl<R, true, MASK_LANE>(const u64*, u64*, const LaneDesc*, StepParams, LtlArgs, TileArgs);
LTL_SPLIT(1) LTL_SPLIT(2) LTL_SPLIT(3) LTL_SPLIT(4) LTL_SPLIT(5) LTL_SPLIT(6) LTL_SPLIT(7)
#undef LTL_SPLIT
#endif

const void* ltl_kernel_of(int range, bool bounded) {
    switch (range) {
#define RANGE_CASE(R) \
    case R:           \
        return bounded ? (const void*)step_ltl<R, true, 0> : (const void*)step_ltl<R, false, 0>;
        RANGE_CASE(1) RANGE_CASE(2) RANGE_CASE(3) RANGE_CASE(4) RANGE_CASE(5) RANGE_CASE(6) RANGE_CASE(7)
#undef RANGE_CASE
        default:
            return nullptr;
    }
}

}  // namespace

int ltl_blocks_per_cu(int range, bool bounded) { return blocks_per_cu(ltl_kernel_of(range, bounded)); }

void launch_step_ltl(const Rule& rule, const BoardEdges& place, bool bounded, const u64* src, u64* dst, const LaneDesc* plan,
                     i64 n_waves, const StepParams& p, hipStream_t s) {
    if (!rule.ltl()) throw Error("step_ltl: rule " + rule.str() + " is not a Larger than Life rule");
    const int R = rule.range;
    const void* f = ltl_kernel_of(R, bounded);
    if (!f) throw Error(strprintf("no Larger than Life kernel instantiated for range %d (1..%d)", R, Rule::kMaxRange));
    if (p.flags & STEP_SEAM) throw Error("step_ltl has no seam-reading variant (sub-tiles do not run Larger than Life rules)");
    if (!(p.flags & STEP_WRAP_Y))
        throw Error("step_ltl reads its rows modulo the tile's height (STEP_WRAP_Y): Larger than Life rules run on one rank");
    if (p.R < R || p.h < 2 * R + 1 || p.nw < 1)
        throw Error(strprintf("step_ltl: range %d on a tile of %d rows with a halo of %d rows (needs %d rows and a halo of %d)", R,
                              (int)p.h, (int)p.R, 2 * R + 1, R));
    check_place("step_ltl", place);
    const Rule::LtlThresholds t = rule.ltl_thresholds();
    LtlArgs la{t.blo, t.bhi, t.slo, t.shi};
    TileArgs ta = tile_args(&place, 0, p);
    const dim3 grid((unsigned)(n_waves / kWavesPerBlock)), block(64 * kWavesPerBlock);
    StepParams pp = p;
    if (!pp.trash) pp.trash = trash_of_current_device();
    void* args[] = {(void*)&src, (void*)&dst, (void*)&plan, (void*)&pp, (void*)&la, (void*)&ta};
    const hipError_t e = hipLaunchKernel(f, grid, block, args, 0, s);
    if (e != hipSuccess) throw Error(strprintf("ltl kernel launch failed: %s", hipGetErrorString(e)));
}

}  // namespace hipk
}  // namespace gol
