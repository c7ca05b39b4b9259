// gol-mi355x: step_gen's policy (rule_runner.hpp tells what a policy is; generations_kernel.hip explains this one).
#pragma once

#include "rule_runner.hpp"

namespace gol {
namespace hipk {
namespace {

// step_gen's kernel argument: where the decay planes lie and the rule's state count C.
struct GenArgs {
    i64 plane_stride;  // u64 words from a plane to the next, in src and in dst alike: plane m + 1 of the decay counter
                       // starts (m + 1) * plane_stride words after the live plane
    u32 states;        // C, 3 .. 9
};

constexpr unsigned kLutOr3 = lut3([](unsigned a, unsigned b, unsigned c) { return a | b | c; });
constexpr unsigned kLutAndNot = lut3([](unsigned a, unsigned b, unsigned) { return a & ~b; });          // a & ~b
constexpr unsigned kLutAndOr = lut3([](unsigned a, unsigned b, unsigned c) { return a & (b | c); });    // a & (b | c)
constexpr unsigned kLutAndXor = lut3([](unsigned a, unsigned b, unsigned c) { return a & (b ^ c); });   // a & (b ^ c)
constexpr unsigned kLutOrAndNot = lut3([](unsigned a, unsigned b, unsigned c) { return a | (b & ~c); });  // a | (b & ~c)
constexpr unsigned kLutXorOr = lut3([](unsigned a, unsigned b, unsigned c) { return (a ^ b) | c; });    // (a ^ b) | c

// The Tally of the Generations policy: what travels with a row from level l - 1 to level l, one row iteration later
// (the envelope chains' delay, EnvelopeTally): the row's live cells A and its decay counter d as level l - 1 made
// them.  nxt[l] is what level l - 1 made in this row iteration, cur[l] what it made one iteration earlier, which is
// the row level l outputs now.  Level 0 moves nxt to cur at the start of every iteration (renaming in the unrolled
// loop).  Index 0 is not used: level 0's row comes from the policy's load stream.
template <int K, int M>
struct GenTally {
    u32 curA[K][2], nxtA[K][2];
    u32 curD[K][M][2], nxtD[K][M][2];
    __device__ __forceinline__ GenTally() {
#pragma unroll
        for (int l = 0; l < K; ++l)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                curA[l][h] = nxtA[l][h] = 0;
#pragma unroll
                for (int m = 0; m < M; ++m) curD[l][m][h] = nxtD[l][m][h] = 0;
            }
    }
};

// step_gen: the decay counter of a Generations rule travels with its row through the levels.
template <int K, int M, int MASK, bool BOUNDED, int ROWS>
struct GenPolicy {
    static_assert(M >= 1 && M <= 3, "the decay counter has one to three planes (3 <= C <= 9)");
    static constexpr int kRowBarriers = 2;
    // Rows the counter's stream reads ahead: three at every depth, loaded by every input() call, so it reads at most three
    // rows past the segment's last input row.  That lies within what the runner's prefetch already requires of every
    // plane's allocation (three rows at K >= 5, six at K <= 4: the slack rows; ROWS_WRAP wraps).  It is not always a row
    // the runner itself reads: at K <= 4 the runner's tail consumes up to five prefetched rows without loading, and the
    // counter's stream may then be one or two rows ahead of the runner's last load, still inside the three.  (With the
    // runner's six rows at K <= 4 the queue alone took 36 registers at M = 3, and step_gen<2, 3> did not fit 256 VGPRs;
    // docs/PERFORMANCE.md.)
    static constexpr int D = 3;
    static_assert(D <= prefetch_rows<K>(), "the counter's stream reads no further past a segment than the runner's prefetch may");
    EdgeMask<MASK> em;  // BOUNDED
    const uint2* const src1;  // plane 1 of the source, plane 1 of the destination (uniform)
    uint2* const dst1;
    const i64 stride;  // words between planes (uniform)
    const i64 pitch;
    const i32 h;
    u32 last[M];  // bit m of C - 2 as a uniform word: all ones / all zeros
    // The load stream over the decay planes: the runner's addresses (RuleRunner's constructor and next_row), as an
    // index into a plane instead of a pointer.  at: the row of the next load; lrow: its tile row (ROWS_WRAP).
    i64 at;
    int lrow;
    i64 st;  // the index of the next store: where the runner stores the live row
    const bool stores;  // the lane has LANE_STORE (the others store no counter)
    uint2 pf[D][M];
    // The row loaded in the last row iteration (cur: level 0 outputs it now) and in this one (nxt).
    u32 curA[2], nxtA[2], curD[M][2], nxtD[M][2];
    using Tally = GenTally<K, M>;

    __device__ __forceinline__ void next_row() {
        at += pitch;
        if (ROWS == ROWS_WRAP) {  // (RuleRunner::next_row)
            ++lrow;
            const bool w = lrow == h;
            lrow = w ? 0 : lrow;
            at = w ? at - (i64)h * pitch : at;
        }
    }
    __device__ __forceinline__ void load_row(uint2 (&row)[M]) const {
#pragma unroll
        for (int m = 0; m < M; ++m) row[m] = src1[(i64)m * stride + at];
    }

    __device__ __forceinline__ GenPolicy(const LaneDesc& d, int, const StepParams& p, const TileArgs& ta, const u64* src, u64* dst,
                                         const GenArgs& ga)
        : src1(reinterpret_cast<const uint2*>(src + ga.plane_stride)), dst1(reinterpret_cast<uint2*>(dst + ga.plane_stride)),
          stride(ga.plane_stride), pitch(p.pitch), h(p.h), stores(d.flags & LANE_STORE) {
        if (BOUNDED) em.template init<K>(d, ta);
#pragma unroll
        for (int m = 0; m < M; ++m) last[m] = 0u - (((ga.states - 2u) >> m) & 1u);
        lrow = d.row0 - K;
        if (ROWS == ROWS_WRAP && lrow < 0) lrow += p.h;
        at = (i64)(lrow + p.R) * p.pitch + (d.col + 1);
        st = (i64)(d.row0 + p.R) * p.pitch + (d.col + 1);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            curA[h2] = nxtA[h2] = 0;
#pragma unroll
            for (int m = 0; m < M; ++m) curD[m][h2] = nxtD[m][h2] = 0;
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            load_row(pf[j]);
            next_row();
        }
    }

    // The loaded row of row iteration i and, from the policy's own stream, its counter: both wait one iteration for
    // level 0, which outputs the row loaded before this one.  (BOUNDED: the counter is masked as the row is; ghost
    // rows and words hold the torus neighbour's.)
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) {
        if (BOUNDED) em.apply(lo, hi, i);
        curA[0] = nxtA[0], curA[1] = nxtA[1];
        nxtA[0] = lo, nxtA[1] = hi;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            curD[m][0] = nxtD[m][0], curD[m][1] = nxtD[m][1];
            u32 dl = pf[0][m].x, dh = pf[0][m].y;
            if (BOUNDED) em.apply(dl, dh, i);
            nxtD[m][0] = dl, nxtD[m][1] = dh;
        }
#pragma unroll
        for (int j = 0; j + 1 < D; ++j)
#pragma unroll
            for (int m = 0; m < M; ++m) pf[j][m] = pf[j + 1][m];  // (a queue of D rows: renaming in the unrolled code)
        load_row(pf[D - 1]);
        next_row();
    }

    // One word half of a level.  R: the gates' output for the live plane alone; A, d: the row's live cells and counter
    // at the previous level.
    //   A' = R & ~any(d)
    //   d' = (A & ~R) ? 1 : (any(d) & d != C - 2 ? d + 1 : 0)      (A & ~R and any(d) exclude each other)
    __device__ __forceinline__ void half(u32 R, u32 A, const u32 (&d)[M], u32& nA, u32 (&nd)[M]) const {
        const u32 d0 = d[0];
        u32 any, keep;  // keep: dying and not at the last state, any(d) & (d != C - 2)
        if constexpr (M == 1) {
            any = d0;
            keep = b3<kLutAndXor>(d0, d0, last[0]);
        } else if constexpr (M == 2) {
            any = d0 | d[1];
            keep = b3<kLutAndOr>(any, d0 ^ last[0], d[1] ^ last[1]);
        } else {
            any = b3<kLutOr3>(d0, d[1], d[2]);
            keep = b3<kLutAndOr>(any, b3<kLutXorOr>(d0, last[0], d[1] ^ last[1]), d[2] ^ last[2]);
        }
        nA = b3<kLutAndNot>(R, any, any);
        const u32 start = b3<kLutAndNot>(A, R, R);
        nd[0] = b3<kLutOrAndNot>(start, keep, d0);  // d + 1, a ripple over the planes, where the cell keeps dying
        if constexpr (M >= 2) nd[1] = b3<kLutAndXor>(keep, d[1], d0);
        if constexpr (M >= 3) nd[2] = b3<kLutAndXor>(keep, d[2], d0 & d[1]);
    }

    // Level l: the new live cells replace the gates' output in place (the next level's ring sees them, as with the
    // edge mask); the new counter is handed on, or, at the last level, stored where the runner stores the row.
    __device__ __forceinline__ void level(Tally& ty, int l, u32& lo, u32& hi, int t) {
        if (l == 0) {
#pragma unroll
            for (int k = 1; k < K; ++k)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    ty.curA[k][h2] = ty.nxtA[k][h2];
#pragma unroll
                    for (int m = 0; m < M; ++m) ty.curD[k][m][h2] = ty.nxtD[k][m][h2];
                }
        }
        u32 nA[2], nd[2][M];
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            u32 d[M];
#pragma unroll
            for (int m = 0; m < M; ++m) d[m] = l == 0 ? curD[m][h2] : ty.curD[l][m][h2];
            half(h2 == 0 ? lo : hi, l == 0 ? curA[h2] : ty.curA[l][h2], d, nA[h2], nd[h2]);
        }
        if (BOUNDED) {
            em.apply(nA[0], nA[1], t);
#pragma unroll
            for (int m = 0; m < M; ++m) em.apply(nd[0][m], nd[1][m], t);
        }
        lo = nA[0], hi = nA[1];
        if (l + 1 < K) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                ty.nxtA[l + 1][h2] = nA[h2];
#pragma unroll
                for (int m = 0; m < M; ++m) ty.nxtD[l + 1][m][h2] = nd[h2][m];
            }
            return;
        }
        // The last level is called exactly when the runner stores (advance() returns true after it): every stored row
        // of the segment gets its counter, the extension rows a later pass of the superstep reads included.
        if (stores) {
#pragma unroll
            for (int m = 0; m < M; ++m) dst1[(i64)m * stride + st] = make_uint2(nd[0][m], nd[1][m]);
        }
        st += pitch;
    }
};

}  // namespace
}  // namespace hipk
}  // namespace gol
