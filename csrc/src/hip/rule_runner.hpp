// gol-mi355x: what the four generic-rule kernels for gfx950 (CDNA4) share on the device: the rule gates, the level
// loop and the streaming wave of step_rule (rule_kernel.hip), step_rule_bounded (rule_bounded_kernel.hip),
// step_census (census_kernel.hip) and step_signature (signature_kernel.hip), the edge and ownership masks of the
// last three, and their kernel argument.  Each kernel's translation unit adds a policy (below) and nothing else to
// the wave.
//
// Everything but the last gates of a level is step_temporal's (step_kernels.hip): the same plans (LaneDesc: 62
// output + 2 halo lanes per wave, trash slots for lanes that store nothing), the same StepParams, the same load
// stream (wave_runner.hpp's row prefetch and ROWS_GHOST / ROWS_WRAP), the same split word format, hsum_split, DPP
// lane moves and v_bitop3_b32 adders, the same register ring (three slots of s0, s1, x per level and half; no extra
// plane lives across rows).  RuleRunner repeats WaveRunner (wave_runner.hpp) rather than sharing it: sharing it
// through a step-policy template parameter whose default reproduced step_temporal's instantiations changed the
// register allocation of step_kernels.hip's gfx950 code (docs/PERFORMANCE.md "Life-like rules"), so the hot kernel's
// runner stays untouched and the generic kernels share this one among themselves (docs/PERFORMANCE.md section 23).
//
// INVARIANT (what makes the host-side validate_plan sufficient for these kernels too): a kernel built on RuleRunner
// reads and writes exactly the rows and words step_temporal<K> reads and writes for the same plan and StepParams.
// The loads, the stores and their addresses are those of WaveRunner<K, ROWS>, kept line for line: the constructor's
// addresses (load stream from row row0 - K, store pointer or trash slot, strides), next_row's ROWS_WRAP select, the
// prefetch depth prefetch_rows<K>() and with it the rows read past a segment's last input row (3 or 6: the engine's
// slack rows), one store per row from row 2K on.  A policy only changes the register arithmetic between a row's load
// and its store; the memory it touches of its own (the census and signature slots, LDS) is no board memory.  What is
// left out of WaveRunner: ROWS_SEAM (sub-tiles run B3/S23 on the torus only) and the two-triple steady loop (at K = 7
// it took 271 registers in step_rule against 155 with the one-triple loop).
//
// Rule evaluation, per level and word half (v_bitop3_b32's truth table is an immediate, so a run-time rule cannot be
// folded into LUTs):
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
// A policy is what a kernel does to the values that pass through the levels.  It is constructed from the lane's
// LaneDesc, the wave's row count, StepParams and whatever the kernel hands the runner after the gates, and gives:
//   kRowBarriers               which rows of a K = 8 row triple a scheduling barrier follows (bit 0: the first,
//                              bit 1: the second); RuleRunner::run tells what for
//   Tally                      what the wave accumulates over its rows (default-constructed; empty when nothing)
//   input(lo, hi, i)           the loaded row of row iteration i, before level 0
//   level(tally, l, lo, hi, t) the output of level l, a row of the unwrapped row counter t = i - (l + 1)
//   finish(tally, wave_id, out) the end of the wave, called by the kernels whose policy has one
// The policy itself holds what is constant over the wave (masks, keys).  It and the tally are two members of the
// runner because of where they lie: the constants before the load stream's state, the accumulators after the register
// ring, as in the kernels before they shared a runner.  With the accumulators beside the masks the gfx950 code of
// step_census differed from theirs in 25 of 32 instantiations instead of 16 (docs/PERFORMANCE.md section 23).
// The loop counter i IS the unwrapped row counter: the level-j value of row iteration i (j = 0 the loaded row,
// j = l + 1 the output of level l) belongs to the unwrapped tile row  row0 - K + i - j.  (lrow, the ROWS_WRAP load
// row, wraps several times per pass on a 1-, 2- or 3-row board; i does not.)
#pragma once

#include <type_traits>

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

// The rule's two 9-bit masks: run-time, wave-uniform, a kernel argument of their own (StepParams, and with it the
// kernarg layout of every other kernel, is unchanged).
struct RuleMasks {
    u32 birth, survive;
};

// The tile's place on the global board, the board's edges and the tile's own cells (rule_launch.hpp fills it in;
// step_rule_bounded reads the board's edges only, the torus census the own cells only).
struct TileArgs {
    i64 grow0;             // global row of tile row 0
    i64 grows;             // rows of the global board (H)
    i64 gword0;            // global word index of tile word 0
    i64 gwords;            // words per global row, ceil(W / 64)
    u32 tail_lo, tail_hi;  // valid cells of the board's last word, split order (even / odd columns)
    u32 own_lo, own_hi;    // cells of the tile in its word nw - 1, split order
};

// The uniform leaf words of the rule (all ones / all zeros) and the generic finish of a level.
struct RuleGates {
    u32 B[9];  // B[c]: a dead cell with c neighbours is born   (B[0] is 0: refused on the host)
    u32 S[9];  // S[c]: a live cell with c neighbours survives

    __device__ __forceinline__ explicit RuleGates(const RuleMasks& m) {
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
};

// step_rule's policy: nothing.  (An empty member of the runner: [[no_unique_address]] there keeps the runner's
// layout, and with it the K = 7 and 8 register names, what they are without a policy.)
struct NoPolicy {
    static constexpr int kRowBarriers = 0;
    __device__ __forceinline__ NoPolicy(const LaneDesc&, int, const StepParams&) {}
    __device__ __forceinline__ void input(u32&, u32&, int) const {}
    struct Tally {};
    __device__ __forceinline__ void level(Tally&, int, u32&, u32&, int) const {}
};

// A wave that streams one segment (every full-width segment) has one row0: there the row tests of the masks below
// are made scalar with readfirstlane and cost s_sub + s_cmp + s_cselect per level, no VALU (MASK_UNI).  The planner
// packs several narrow segments of the same height, but of different rows, into one wave (plan.cpp pack_waves): such
// a wave keeps the tests' offsets per lane and pays v_sub + v_cmp + v_cndmask per level on top (MASK_LANE: the same
// source, the offset in a VGPR).  A kernel picks the runner per wave, uniformly, with one_row0 below.
// (A third runner without masks for waves that reach no edge was built and measured in step_rule_bounded: slower,
// 32768^2 30.4 against 24.2 us/gen, 8192^2 5.35 against 4.70 -- three unrolled K = 8 loops in one kernel -- so it is
// not here.)
enum { MASK_UNI = 1, MASK_LANE = 2 };

// The in-board cells of the word a lane streams (bounded boards).  The engine builds bounded plans without x-wrap
// (halo lanes stream the ghost words, col = -1 or nw), so a lane's global word index tells whether it is outside.
//   * column mask, per lane, formed once from the global index of the lane's word: all ones inside the board, the
//     tail mask (split order) on the board's last word, zero beyond either edge;
//   * row mask, per level: row counter t is on the board iff  (u32)(t - A) < span  with  A = row_lo - row0 + K,
//     row_lo the tile row of global row 0 and span the board's rows.
// A level's value is then  x & colmask & rowmask: one v_bitop3 (and3) per word half.
template <int MASK>
struct EdgeMask {
    u32 col_lo, col_hi;
    int A;
    u32 span;

    template <int K>
    __device__ __forceinline__ void init(const LaneDesc& d, const TileArgs& ta) {
        const i64 gw = ta.gword0 + d.col;
        const bool inside = gw >= 0 && gw < ta.gwords, last = gw == ta.gwords - 1;
        col_lo = inside ? (last ? ta.tail_lo : ~0u) : 0u;
        col_hi = inside ? (last ? ta.tail_hi : ~0u) : 0u;
        // rows of the board in tile coordinates, clamped far outside anything a pass touches (|rows| < 2^30)
        constexpr i64 kFar = (i64)1 << 30;
        const i64 lo64 = -ta.grow0 < -kFar ? -kFar : -ta.grow0;
        const i64 hi64 = ta.grows - ta.grow0 > kFar ? kFar : ta.grows - ta.grow0;
        span = (u32)(hi64 - lo64);
        const int a = (int)lo64 - d.row0 + K;
        A = MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(a) : a;
    }

    __device__ __forceinline__ void apply(u32& lo, u32& hi, int t) const {
        const u32 r = (u32)(t - A) < span ? ~0u : 0u;
        lo = b3<kLutAnd3>(lo, col_lo, r);
        hi = b3<kLutAnd3>(hi, col_hi, r);
    }
};

// The cells a lane owns: counted or hashed once per generation (census_kernel.hip tells why these partition the
// tile).  A store lane's word of the tile (the tile's storage mask on word nw - 1), rows of the segment inside the
// tile:  max(row0, 0) <= t < min(row0 + nrows, h)  as  (u32)(t - Ao) < ospan  with  Ao = max(row0, 0) - row0 + K.
template <int MASK>
struct OwnMask {
    u32 own_lo, own_hi;  // owned cells of the lane's word (0 for lanes that own nothing)
    int Ao;
    u32 ospan;

    // stores: the lane has LANE_STORE.  (owns is formed in two steps: as one && chain the compiler orders the
    // prologue's compares otherwise, and with them the registers of the whole kernel; section 23.)
    template <int K>
    __device__ __forceinline__ void init(bool stores, const LaneDesc& d, int nrows, const StepParams& p, const TileArgs& ta) {
        const bool left = stores && d.col >= 0;
        const bool owns = left && d.col < p.nw, tail = d.col == p.nw - 1;
        own_lo = owns ? (tail ? ta.own_lo : ~0u) : 0u;
        own_hi = owns ? (tail ? ta.own_hi : ~0u) : 0u;
        const int olo = d.row0 > 0 ? d.row0 : 0;
        const int ohi = d.row0 + nrows < p.h ? d.row0 + nrows : p.h;
        const int ao = olo - d.row0 + K;
        const u32 os = ohi > olo ? (u32)(ohi - olo) : 0u;
        Ao = MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(ao) : ao;
        ospan = MASK == MASK_UNI ? (u32)__builtin_amdgcn_readfirstlane((int)os) : os;
    }

    // all ones when row counter t is an owned row
    __device__ __forceinline__ u32 row(int t) const { return (u32)(t - Ao) < ospan ? ~0u : 0u; }
};

// The Tally of the census and signature policies: the lane's count of owned live cells, per level.
template <int K>
struct CountTally {
    u32 acc[K];
    __device__ __forceinline__ CountTally() {
#pragma unroll
        for (int l = 0; l < K; ++l) acc[l] = 0;
    }
};

// hsum_split (stencil_device.hpp, step_temporal's: left as it is) that also hands out the two shifted words it
// forms: Le, the left neighbours of the even cells, and Ro, the right neighbours of the odd cells.
__device__ __forceinline__ void hsum_split_lr(u32 lo, u32 hi, u32& s0lo, u32& s1lo, u32& s0hi, u32& s1hi, u32& Le, u32& Ro) {
    const u32 ph = dpp_prev(hi), nl = dpp_next(lo);
    Le = __builtin_amdgcn_alignbit(hi, ph, 31);  // (hi << 1) | (ph >> 31)
    Ro = __builtin_amdgcn_alignbit(nl, lo, 1);   // (lo >> 1) | (nl << 31)
    s0lo = b3<kLutXor3>(Le, lo, hi);
    s1lo = b3<kLutMaj>(Le, lo, hi);
    s0hi = b3<kLutXor3>(lo, hi, Ro);
    s1hi = b3<kLutMaj>(lo, hi, Ro);
}

// The streaming wave: one wave streams one plan segment through the K levels and stores its output rows.
// Gates is the neighbourhood: RuleGates (Moore; the default, and the code of this header), or the von Neumann or
// hexagonal gates of nbhd_gates.hpp, which finish a level from the same register ring (advance tells how).  The
// Moore path stands inside `if constexpr` as it stood before there were other gates: its instantiations' gfx950
// code is what it was (docs/PERFORMANCE.md section 24).
template <int K, int ROWS, class Policy, class Gates = RuleGates>
struct RuleRunner {
    static_assert(ROWS == ROWS_GHOST || ROWS == ROWS_WRAP, "the generic-rule kernels read ghost rows or wrap");
    static constexpr int D = prefetch_rows<K>();
    const Gates step;
    const StepParams& p;
    const LaneDesc& d;
    const int n;   // row iterations: nrows + 2K
    const i64 hp;  // h * pitch
    [[no_unique_address]] Policy policy;
    const uint2* ld;
    uint2* st;
    i64 st_stride;  // pitch for output lanes, 0 for halo/idle lanes (they write a trash slot)
    int lrow;       // tile row of the next load (ROWS_WRAP; wave-uniform)
    uint2 pf[D];
    Pipe<K> P;
    [[no_unique_address]] typename Policy::Tally tally;

    __device__ __forceinline__ void next_row() {
        ld += p.pitch;
        if (ROWS == ROWS_WRAP) {  // rows are periodic: row h is row 0 (branch-free select)
            ++lrow;
            const bool w = lrow == p.h;
            lrow = w ? 0 : lrow;
            ld = w ? ld - hp : ld;
        }
    }

    template <class... A>
    __device__ __forceinline__ RuleRunner(const u64* src, u64* dst, const LaneDesc& d_, int nrows, const StepParams& p_,
                                          i64 wave_id, const Gates& step_, const A&... policy_args)
        : step(step_), p(p_), d(d_), n(nrows + 2 * K), hp((i64)p_.h * p_.pitch), policy(d_, nrows, p_, policy_args...) {
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

    // Push one row through the K levels: advance() of stencil_device.hpp without the pair mode, with the rule
    // gates as the finish and the policy on every level's output.  Same ring, same slots, same fill-phase guards.
    template <int PH, bool GUARD>
    __device__ __forceinline__ bool advance(u32& lo, u32& hi, int i) {
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (GUARD && i < 2 * l) return false;
            const int s = (PH + l) % 3;   // slot of the arriving row
            const int sp = (s + 2) % 3;   // previous row (centre of the output)
            const int spp = (s + 1) % 3;  // two rows back
            if constexpr (std::is_same<Gates, RuleGates>::value) {
                hsum_split(lo, hi, P.s0[l][s][0], P.s1[l][s][0], P.s0[l][s][1], P.s1[l][s][1]);
                P.x[l][s][0] = lo;
                P.x[l][s][1] = hi;
                if (GUARD && i < 2 * l + 2) return false;
                lo = step.rule(P.s0[l][spp][0], P.s1[l][spp][0], P.s0[l][sp][0], P.s1[l][sp][0], P.s0[l][s][0],
                               P.s1[l][s][0], P.x[l][sp][0]);
                hi = step.rule(P.s0[l][spp][1], P.s1[l][spp][1], P.s0[l][sp][1], P.s1[l][sp][1], P.s0[l][s][1],
                               P.s1[l][s][1], P.x[l][sp][1]);
            } else {
                // other neighbourhoods: the gates take the arriving row's shifted words too (used at once), and
                // read the rows above and below the centre from the ring's x, not from their horizontal sums
                u32 Le, Ro;
                hsum_split_lr(lo, hi, P.s0[l][s][0], P.s1[l][s][0], P.s0[l][s][1], P.s1[l][s][1], Le, Ro);
                P.x[l][s][0] = lo;
                P.x[l][s][1] = hi;
                if (GUARD && i < 2 * l + 2) return false;
                step.next(P, l, s, sp, spp, Le, Ro, lo, hi);
            }
            policy.level(tally, l, lo, hi, i - (l + 1));
        }
        return true;
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
        policy.input(lo, hi, i);
        if (!advance<PH, GUARD>(lo, hi, i)) return;
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
                // K = 8 with masks (Policy::kRowBarriers = 2): a scheduling barrier keeps the third row of a triple
                // apart from the first two.  Left free, the scheduler interleaves the three rows' level chains and
                // step_rule_bounded's steady loop takes 256 VGPRs plus AGPR copies, 1 wave per SIMD (32768^2: 37.9
                // us/gen against the torus kernel's 22.7); with the one barrier 184 / 255 VGPRs, 2 waves as
                // step_rule<8> (24.2); a barrier after each of the two rows costs the overlap of the rows' chains
                // (28.7).  docs/PERFORMANCE.md "Bounded boards".
                compute_store<0, false>(x0.x, x0.y, i);
                if constexpr (K >= 8 && (Policy::kRowBarriers & 1)) __builtin_amdgcn_sched_barrier(0);
                compute_store<1, false>(x1.x, x1.y, i + 1);
                if constexpr (K >= 8 && (Policy::kRowBarriers & 2)) __builtin_amdgcn_sched_barrier(0);
                compute_store<2, false>(x2.x, x2.y, i + 2);
            }
            if (i < n) body<0, false>(i);
            if (i + 1 < n) body<1, false>(i + 1);
        }
    }
};

// One segment per wave, or packed segments of the same rows: the wave runs the MASK_UNI runner.  (The two runners
// are instantiated in the kernels, not in a shared function around them: such a function changed the gfx950 code
// of all 16 step_rule_bounded instantiations; docs/PERFORMANCE.md section 23.)
__device__ __forceinline__ bool one_row0(const LaneDesc& d) {
    return __builtin_amdgcn_ballot_w64(d.row0 != __builtin_amdgcn_readfirstlane(d.row0)) == 0;
}

}  // namespace
}  // namespace hipk
}  // namespace gol
