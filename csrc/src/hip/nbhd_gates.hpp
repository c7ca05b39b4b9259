// gol-mi355x: the von Neumann and hexagonal rule gates of the generic-rule kernels for gfx950 (CDNA4), beside the
// Moore RuleGates of rule_runner.hpp, and what the kernels of the nbhd_*.hip units share: the neighbourhood dispatch.
//
// A neighbourhood changes only the gates between a row's load and its store: RuleRunner<K, ROWS, Policy, Gates> with
// one of these gates is the same streaming wave (the same loads, stores, prefetch depth and trash slots, so the
// invariant of rule_runner.hpp and with it validate_plan cover these kernels too), the same policies and the same
// register ring: three slots of s0, s1, x per level and half, no extra plane.  Both evaluate
//     F = x ? S[T - 1] : B[T],   T the neighbourhood sum INCLUDING the centre
// as a mux tree over the planes of T, with the leaves  leaf_T = x ? S[T - 1] : B[T]  of RuleGates.  With the rows
// a (above, ring slot spp), b (centre, sp) and c (arriving, s):
//
// von Neumann (N, S, W, E; T = 0..5):  T = x_a + hsum(b) + x_c, hsum(b) = (b0, b1) the ring's horizontal sum of
// the centre row (centre included).  Per word half and level, 13 v_bitop3 against Moore's 24:
//     t0 = xor3(x_a, b0, x_c), cy = maj(x_a, b0, x_c), t1 = b1 ^ cy, t2 = b1 & cy                     4
//     leaf_1 .. leaf_4                                                                                4
//     m01 = t0 & leaf_1, m23 = t0 ? leaf_3 : leaf_2, m45 = t0 ? S[4] : leaf_4  (T = 5 has x = 1),
//     q = t1 ? m23 : m01, F = t2 ? m45 : q  (T >= 4: t1 = 0)                                          5
// With the 4 of the horizontal sum 17 against 28.  The sums of rows a and c are not read: the ring's s0, s1 live
// from a row's arrival to its turn as the centre, two slots of three.
//
// hexagonal (N, S, W, E, NW, SE; T = 0..7):  T = (l + x)_a + hsum(b) + (x + r)_c, l / r a row's left / right
// neighbours.  The split word format makes the halves differ:
//     even cells:  l_a = Le of row a (the odd half shifted, a lane move),   r_c = the same bit of c's odd half
//     odd cells:   l_a = the same bit of a's even half,                     r_c = Ro of row c (formed on arrival)
// Ro of the arriving row is used at once (hsum_split_lr hands it out).  Le of row a is needed two rows after
// hsum_split formed it.  It is recovered from the ring:  s0 = Le ^ lo ^ hi, so  Le = xor3(s0_a, lo_a, hi_a), one
// v_bitop3 on the even half, and the even half's s0 stays live for its third slot.  (A stored plane, 3 K registers,
// and forming Le again with a lane move and a v_alignbit were built too: at K = 8 either puts step_rule_bounded and
// step_census past 256 registers; docs/PERFORMANCE.md section 24 has the three sets of counts.)  Per word half and
// level, 19 v_bitop3 (even half: 20):
//     u = xor3(l_a, x_a, b0), c1 = maj(l_a, x_a, b0), t0 = xor3(u, x_c, r_c), c2 = maj(u, x_c, r_c),
//     t1 = xor3(b1, c1, c2), t2 = maj(b1, c1, c2)                                                     6
//     leaf_1 .. leaf_6                                                                                6
//     m01 = t0 & leaf_1, m23, m45, m67 = t0 ? S[6] : leaf_6  (T = 7 has x = 1), q0, q1, F             7
// With the 4 of the horizontal sum 23 / 24 against 28.
#pragma once

#include "rule_launch.hpp"

namespace gol {
namespace hipk {
namespace {

struct VonNeumannGates {
    u32 B[5];  // B[c]: a dead cell with c neighbours is born   (B[0] is 0: refused on the host)
    u32 S[5];  // S[c]: a live cell with c neighbours survives

    __device__ __forceinline__ explicit VonNeumannGates(const RuleMasks& m) {
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            B[c] = 0u - ((m.birth >> c) & 1u);
            S[c] = 0u - ((m.survive >> c) & 1u);
        }
    }

    template <int T>
    __device__ __forceinline__ u32 leaf(u32 x) const {
        return b3<kLutMux>(x, S[T - 1], B[T]);
    }

    // next state of 32 cells from the cells above (a) and below (c), the centre row's horizontal sum and the centre
    __device__ __forceinline__ u32 rule(u32 a, u32 b0, u32 b1, u32 c, u32 x) const {
        const u32 t0 = b3<kLutXor3>(a, b0, c);
        const u32 cy = b3<kLutMaj>(a, b0, c);
        const u32 t1 = b3<kLutXor2>(b1, cy, cy);
        const u32 t2 = b3<kLutAnd2>(b1, cy, cy);
        const u32 m01 = b3<kLutAnd2>(t0, leaf<1>(x), x);
        const u32 m23 = b3<kLutMux>(t0, leaf<3>(x), leaf<2>(x));
        const u32 m45 = b3<kLutMux>(t0, S[4], leaf<4>(x));  // T = 5 has a live centre
        const u32 q = b3<kLutMux>(t1, m23, m01);
        return b3<kLutMux>(t2, m45, q);  // T >= 4: t1 = 0
    }

    template <int K>
    __device__ __forceinline__ void next(const Pipe<K>& P, int l, int s, int sp, int spp, u32, u32, u32& lo, u32& hi) const {
        lo = rule(P.x[l][spp][0], P.s0[l][sp][0], P.s1[l][sp][0], P.x[l][s][0], P.x[l][sp][0]);
        hi = rule(P.x[l][spp][1], P.s0[l][sp][1], P.s1[l][sp][1], P.x[l][s][1], P.x[l][sp][1]);
    }
};

struct HexGates {
    u32 B[7];
    u32 S[7];

    __device__ __forceinline__ explicit HexGates(const RuleMasks& m) {
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            B[c] = 0u - ((m.birth >> c) & 1u);
            S[c] = 0u - ((m.survive >> c) & 1u);
        }
    }

    template <int T>
    __device__ __forceinline__ u32 leaf(u32 x) const {
        return b3<kLutMux>(x, S[T - 1], B[T]);
    }

    // next state of 32 cells from two cells of the row above (a1, a2), the centre row's horizontal sum, two cells of
    // the row below (c1, c2) and the centre
    __device__ __forceinline__ u32 rule(u32 a1, u32 a2, u32 b0, u32 b1, u32 c1, u32 c2, u32 x) const {
        const u32 u = b3<kLutXor3>(a1, a2, b0);
        const u32 k1 = b3<kLutMaj>(a1, a2, b0);
        const u32 t0 = b3<kLutXor3>(u, c1, c2);
        const u32 k2 = b3<kLutMaj>(u, c1, c2);
        const u32 t1 = b3<kLutXor3>(b1, k1, k2);
        const u32 t2 = b3<kLutMaj>(b1, k1, k2);
        const u32 m01 = b3<kLutAnd2>(t0, leaf<1>(x), x);
        const u32 m23 = b3<kLutMux>(t0, leaf<3>(x), leaf<2>(x));
        const u32 m45 = b3<kLutMux>(t0, leaf<5>(x), leaf<4>(x));
        const u32 m67 = b3<kLutMux>(t0, S[6], leaf<6>(x));  // T = 7 has a live centre
        const u32 q0 = b3<kLutMux>(t1, m23, m01);
        const u32 q1 = b3<kLutMux>(t1, m67, m45);
        return b3<kLutMux>(t2, q1, q0);
    }

    template <int K>
    __device__ __forceinline__ void next(const Pipe<K>& P, int l, int s, int sp, int spp, u32, u32 Ro, u32& lo, u32& hi) const {
        const u32 alo = P.x[l][spp][0], ahi = P.x[l][spp][1];
        const u32 Le = b3<kLutXor3>(P.s0[l][spp][0], alo, ahi);  // s0 = Le ^ lo ^ hi (the header tells why not a plane)
        const u32 clo = P.x[l][s][0], chi = P.x[l][s][1];
        lo = rule(Le, alo, P.s0[l][sp][0], P.s1[l][sp][0], clo, chi, P.x[l][sp][0]);
        hi = rule(alo, ahi, P.s0[l][sp][1], P.s1[l][sp][1], chi, Ro, P.x[l][sp][1]);
    }
};

// The kernel of a family for the rule's neighbourhood: of(gates) returns the instantiation's address for a
// default-constructible tag of the gates type.
template <class G>
struct GatesTag {
    using type = G;
};

template <class F>
const void* nbhd_kernel_of(Nbhd nbhd, F of) {
    switch (nbhd) {
        case Nbhd::VonNeumann:
            return of(GatesTag<VonNeumannGates>{});
        case Nbhd::Hex:
            return of(GatesTag<HexGates>{});
        default:
            return nullptr;  // Moore: the kernels of rule_kernel.hip and its siblings
    }
}

}  // namespace
}  // namespace hipk
}  // namespace gol
