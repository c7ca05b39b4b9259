// gol-mi355x: the policies of step_rule_bounded, step_census, step_signature and step_film (rule_runner.hpp tells what
// a policy is), in a header because each has two kernels: the Moore one in rule_bounded_kernel.hip, census_kernel.hip,
// signature_kernel.hip and film_kernel.hip, whose headers explain the policies, and the von Neumann / hexagonal one in
// the nbhd_*.hip unit of the same family.
#pragma once

#include "gol/signature.hpp"
#include "rule_runner.hpp"

namespace gol {
namespace hipk {
namespace {

// step_rule_bounded: the edge mask on the loaded row and on every level's output.
template <int K, int MASK>
struct EdgePolicy {
    static constexpr int kRowBarriers = 2;
    EdgeMask<MASK> em;

    __device__ __forceinline__ EdgePolicy(const LaneDesc& d, int, const StepParams&, const TileArgs& ta) {
        em.template init<K>(d, ta);
    }
    // the loaded row: ghost rows and ghost words hold the torus neighbour's cells
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) const { em.apply(lo, hi, i); }
    struct Tally {};
    __device__ __forceinline__ void level(Tally&, int, u32& lo, u32& hi, int t) const { em.apply(lo, hi, t); }
};

// step_census: the count of the owned live cells of every level's output.
template <int K, int MASK, bool BOUNDED>
struct CensusPolicy {
    static constexpr int kRowBarriers = 2;
    EdgeMask<MASK> em;  // BOUNDED
    OwnMask<MASK> own;
    using Tally = CountTally<K>;

    __device__ __forceinline__ CensusPolicy(const LaneDesc& d, int nrows, const StepParams& p, const TileArgs& ta) {
        const bool stores = d.flags & LANE_STORE;  // (ahead of the masks: the prologue's order, PERFORMANCE.md section 23)
        if (BOUNDED) em.template init<K>(d, ta);
        own.template init<K>(stores, d, nrows, p, ta);
    }

    // (BOUNDED) the loaded row: ghost rows and words hold the torus neighbour's cells
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) const {
        if (BOUNDED) em.apply(lo, hi, i);
    }
    // the (masked) output of level l is counted into acc[l]
    __device__ __forceinline__ void level(Tally& ty, int l, u32& lo, u32& hi, int t) const {
        if (BOUNDED) em.apply(lo, hi, t);
        const u32 r = own.row(t);
        ty.acc[l] = (u32)__builtin_popcount(b3<kLutAnd3>(hi, own.own_hi, r)) + ty.acc[l];
        ty.acc[l] = (u32)__builtin_popcount(b3<kLutAnd3>(lo, own.own_lo, r)) + ty.acc[l];
    }
    // The wave's count of each level: summed over the lanes, one 64-bit atomic per level from lane 0.
    __device__ __forceinline__ void finish(const Tally& ty, i64 wave_id, u64* counts) const {
        if (!counts) return;
        const size_t stripe = (size_t)(wave_id & (kCensusStripes - 1)) * kCensusStripeWords;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            u32 v = ty.acc[l];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((threadIdx.x & 63) == 0 && v != 0)
                atomicAdd(reinterpret_cast<unsigned long long*>(counts + (size_t)l * kCensusSlotWords + stripe), (unsigned long long)v);
        }
    }
};

// step_signature: the census, and the hash of every level's output.
template <int K, int MASK, bool BOUNDED>
struct SigPolicy {
    static constexpr int kRowBarriers = 2;
    EdgeMask<MASK> em;  // BOUNDED
    OwnMask<MASK> own;
    u32 gam_e, gam_o;  // column keys of the lane's word
    u32 growb;         // (u32) global row of row counter t = 0: grow0 + row0 - K
    unsigned long long* const sig;  // LDS: level l's accumulator of this lane at sig[l * block size]
    using Tally = CountTally<K>;

    __device__ __forceinline__ SigPolicy(const LaneDesc& d, int nrows, const StepParams& p, const TileArgs& ta,
                                         unsigned long long* lds)
        : sig(lds + threadIdx.x) {
        const bool stores = d.flags & LANE_STORE;  // (ahead of the masks: the prologue's order, PERFORMANCE.md section 23)
        if (BOUNDED) em.template init<K>(d, ta);
        own.template init<K>(stores, d, nrows, p, ta);
        // the keys: the lane's two column keys, and the global row of row counter 0
        const u32 gw2 = 2u * (u32)(ta.gword0 + d.col);
        gam_e = sig_gam(gw2);
        gam_o = sig_gam(gw2 + 1u);
        const int gb = (int)(u32)(ta.grow0 + (i64)d.row0 - K);
        growb = (u32)(MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(gb) : gb);
#pragma unroll
        for (int l = 0; l < K; ++l) sig[l * (64 * kWavesPerBlock)] = 0;
    }

    // The key of the global row of row counter t, a value of its own at every use (signature_kernel.hip's header tells why).
    __device__ __forceinline__ u32 row_key(int t) const {
        if (MASK == MASK_UNI) {
            u32 r = sig_rho(growb + (u32)t);
            asm volatile("" : "+s"(r));
            return r;
        }
        asm volatile("" : "+s"(t));
        return sig_rho(growb + (u32)t);
    }

    // (BOUNDED) the loaded row: ghost rows and words hold the torus neighbour's cells
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) const {
        if (BOUNDED) em.apply(lo, hi, i);
    }
    // the (masked) output of level l is counted into acc[l] and hashed into the lane's LDS slot of level l
    __device__ __forceinline__ void level(Tally& ty, int l, u32& lo, u32& hi, int t) const {
        if (BOUNDED) em.apply(lo, hi, t);
        const u32 rho = row_key(t);
        const u32 r = own.row(t);
        const u32 o = b3<kLutAnd3>(hi, own.own_hi, r);
        const u32 e = b3<kLutAnd3>(lo, own.own_lo, r);
        ty.acc[l] = (u32)__builtin_popcount(o) + ty.acc[l];
        ty.acc[l] = (u32)__builtin_popcount(e) + ty.acc[l];
        const u64 p = (u64)e * (u64)(rho * gam_e) + (u64)o * (u64)(rho * gam_o);
        atomicAdd(sig + l * (64 * kWavesPerBlock), (unsigned long long)p);  // (the lane's own slot: a ds_add_u64 without return)
    }
    // The wave's count and signature of each level: summed over the lanes, two 64-bit atomics per level from lane 0.
    __device__ __forceinline__ void finish(const Tally& ty, i64 wave_id, u64* slots) const {
        if (!slots) return;
        const size_t stripe = (size_t)(wave_id & (kSigStripes - 1)) * kSigStripeWords;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            u32 v = ty.acc[l];
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

// step_film's kernel argument: where the frames of the pass go and which cells are the window's (gol/film.hpp).
struct FilmArgs {
    uint2* frames;   // the slot of the pass's first generation (device memory; nullptr: store nothing)
    u32 slot_words;  // u64 words from one generation's frame to the next: rows * fw
    u32 rows, fw;    // the frame: window rows x board words
    i32 r0, w0;      // board row and board word of frame row 0, frame word 0 (inside the board)
};

// step_film: the owned words of every level's output that lie in the window go to the level's frame.
template <int K, int MASK, bool BOUNDED>
struct FilmPolicy {
    static constexpr int kRowBarriers = 2;
    EdgeMask<MASK> em;  // BOUNDED
    OwnMask<MASK> own;
    uint2* const frames;  // (uniform)
    const u32 slot_words, rows, fw;
    u32 widx;  // the lane's word in a frame row; kNoWord: the lane owns no word of the window
    int d0;    // board row of row counter t = 0, less the window's first row: grow0 + row0 - K - r0
    int H;     // rows of the board
    static constexpr u32 kNoWord = ~0u;
    struct Tally {};

    __device__ __forceinline__ FilmPolicy(const LaneDesc& d, int nrows, const StepParams& p, const TileArgs& ta,
                                          const FilmArgs& fa)
        : frames(fa.frames), slot_words(fa.slot_words), rows(fa.rows), fw(fa.fw) {
        const bool stores = d.flags & LANE_STORE;  // (ahead of the masks: the prologue's order, PERFORMANCE.md section 23)
        if (BOUNDED) em.template init<K>(d, ta);
        own.template init<K>(stores, d, nrows, p, ta);
        // the lane's word: an owned word of the tile is a word of the board, (gword - w0) mod gwords its place in a frame row
        int f = (int)(ta.gword0 + d.col) - fa.w0;
        f += f < 0 ? (int)ta.gwords : 0;
        const bool owns = (own.own_lo | own.own_hi) != 0;
        widx = owns && (u32)f < fa.fw ? (u32)f : kNoWord;
        const int db = (int)(ta.grow0 + (i64)d.row0 - K) - fa.r0;
        d0 = MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(db) : db;
        H = (int)ta.grows;
    }

    // (BOUNDED) the loaded row: ghost rows and words hold the torus neighbour's cells
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) const {
        if (BOUNDED) em.apply(lo, hi, i);
    }
    // The (masked) output of level l: an owned row is a row of the tile, so of the board, and its distance from the
    // window's first row is d0 + t or, before that row, H more: the row test and the frame row at once.
    __device__ __forceinline__ void level(Tally&, int l, u32& lo, u32& hi, int t) const {
        if (BOUNDED) em.apply(lo, hi, t);
        if (!frames) return;  // (uniform)
        int dist = d0 + t;
        dist += dist < 0 ? H : 0;
        if ((u32)(t - own.Ao) < own.ospan && (u32)dist < rows && widx != kNoWord)
            frames[(u32)l * slot_words + (u32)dist * fw + widx] = make_uint2(lo & own.own_lo, hi & own.own_hi);
    }
};

}  // namespace
}  // namespace hipk
}  // namespace gol
