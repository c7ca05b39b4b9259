// gol-mi355x: the policies of step_rule_bounded, step_census, step_signature, step_film, step_density and
// step_envelope (rule_runner.hpp tells what a policy is), in a header because each has two kernels: the Moore one in
// rule_bounded_kernel.hip, census_kernel.hip, signature_kernel.hip, film_kernel.hip, density_kernel.hip and
// envelope_kernel.hip, whose headers explain the policies, and the von Neumann / hexagonal one in the nbhd_*.hip unit
// of the same family.
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

// step_density's kernel argument: where the maps of the pass go and the blocks they count (gol/density_film.hpp).
struct DensityArgs {
    u32* maps;                      // the slot of the pass's first generation (device memory; nullptr: count nothing)
    u32 slot;                       // u32 counts from one generation's map to the next (even)
    u32 block_rows, rows_recip;     // rows of a block and div_recip's reciprocal of them
    u32 block_words, words_recip;   // board words of a block likewise
    u32 grid_cols;                  // blocks in a row of the grid
};

// div_recip's m for the divisor d >= 1: floor(2^32 / d), 2^32 - 1 for d = 1.
inline u32 recip_of(u32 d) { return d <= 1 ? ~0u : (u32)(((u64)1 << 32) / d); }

// n / d for any u32 n, without a division: n m / 2^32 lies below n / d by less than n / 2^32 < 1, so the high word of
// n m is the quotient or one less and one correction makes it exact.  rem: n mod d.  (Scalar where n is uniform.)
__device__ __forceinline__ u32 div_recip(u32 n, u32 d, u32 m, u32& rem) {
    u32 q = __umulhi(n, m);
    rem = n - q * d;
    const bool up = rem >= d;
    rem -= up ? d : 0u;
    return q + (up ? 1u : 0u);
}

// step_density: the census's count of every level's output, flushed into the level's map at every block end.
template <int K, int MASK, bool BOUNDED>
struct DensityPolicy {
    static constexpr int kRowBarriers = 2;
    EdgeMask<MASK> em;  // BOUNDED
    OwnMask<MASK> own;
    u32* const maps;  // (uniform)
    const u32 slot, block_rows, rows_recip, grid_cols;
    const bool pre;  // blocks of several words: lanes of one block column add up before the atomic (uniform)
    u32 bcol;  // the block column of the lane's word (a word lies in one: block_cols is a multiple of 64)
    u32 gb;    // (u32) global row of row counter t = 0: grow0 + row0 - K
    // The row phase (scalar in a MASK_UNI wave, per lane in a MASK_LANE one).  phase: the place in its block row of
    // level 0's row.  ends: bit m says that level m's row of this row iteration is the last of its block row; level
    // m meets the row level 0 met m iterations ago, so the bits move up by one per row and one test serves K levels.
    u32 phase, ends;
    u32 run;   // MASK_UNI: bit k: the lanes up to lane + 2^k hold the lane's block column; bit 6: the lane is the first of its run
    int lane4;  // 4 * lane: ds_bpermute's address of the lane itself
    using Tally = CountTally<K>;
    static constexpr u32 kNoKey = ~0u;

    __device__ __forceinline__ DensityPolicy(const LaneDesc& d, int nrows, const StepParams& p, const TileArgs& ta,
                                             const DensityArgs& da)
        : maps(da.maps), slot(da.slot), block_rows(da.block_rows), rows_recip(da.rows_recip), grid_cols(da.grid_cols),
          pre(da.block_words > 1), ends(0) {
        const bool stores = d.flags & LANE_STORE;  // (ahead of the masks: the prologue's order, PERFORMANCE.md section 23)
        if (BOUNDED) em.template init<K>(d, ta);
        own.template init<K>(stores, d, nrows, p, ta);
        u32 rem;
        bcol = div_recip((u32)(ta.gword0 + d.col), da.block_words, da.words_recip, rem);  // (used by owning lanes only)
        const int g = (int)(u32)(ta.grow0 + (i64)d.row0 - K);
        gb = (u32)(MASK == MASK_UNI ? __builtin_amdgcn_readfirstlane(g) : g);
        // The phase of row counter t = 1, level 0's row at its first call (row iteration 2), counted back from the
        // first owned row Ao >= K >= 1, a row of the board: (gb + Ao) mod block_rows less (Ao - 1) mod block_rows.
        // (Before the first owned row gb + t may be negative; the phase there only has to run on to the right one.)
        u32 pa, pb;
        div_recip(gb + (u32)own.Ao, block_rows, rows_recip, pa);
        div_recip((u32)own.Ao - 1u, block_rows, rows_recip, pb);
        phase = pa >= pb ? pa - pb : pa + block_rows - pb;
        lane4 = (int)(threadIdx.x & 63) * 4;
        // (one row0: the lanes of a block column flush into one block, so the runs are known here)
        run = MASK == MASK_UNI ? runs_of((own.own_lo | own.own_hi) != 0 ? bcol : kNoKey) : 0u;
    }

    // The runs of consecutive lanes with one key (run's layout).  All 64 lanes are active where this is called.
    __device__ __forceinline__ u32 runs_of(u32 key) const {
        // bit 0: the next lane holds the key; bit k: so do all lanes up to lane + 2^k, that is up to lane + 2^(k-1) and
        // from there as far again (a packed wave may hold the same key in two runs with other lanes between them)
        u32 r = (lane4 + 4 < 256 && (u32)__builtin_amdgcn_ds_bpermute(lane4 + 4, (int)key) == key) ? 1u : 0u;
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            const u32 other = (u32)__builtin_amdgcn_ds_bpermute(lane4 + (2 << k), (int)r);  // lane + 2^(k-1)
            r |= ((r & other) >> (k - 1) & 1u) << k;  // (bit k - 1 of r: that lane is in the wave)
        }
        const u32 before = (u32)__builtin_amdgcn_ds_bpermute(lane4 - 4, (int)key);
        return r | ((lane4 == 0 || before != key) ? 64u : 0u);
    }
    // The sum of v over the lanes of the run r describes, in the run's first lane; 0 in the others.  (All lanes active.)
    __device__ __forceinline__ u32 run_sum(u32 v, u32 r) const {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const u32 other = (u32)__builtin_amdgcn_ds_bpermute(lane4 + (4 << k), (int)v);
            v += (r >> k) & 1u ? other : 0u;
        }
        return r & 64u ? v : 0u;
    }

    // level l's count of the lane goes to block (brow, bcol) of the level's map and starts again
    __device__ __forceinline__ void flush(Tally& ty, int l, u32 brow) const {
        if (ty.acc[l] != 0) atomicAdd(maps + ((u32)l * slot + brow * grid_cols + bcol), ty.acc[l]);
        ty.acc[l] = 0;
    }

    // The start of a row iteration whose level 0 has row counter t (level 0 is called first, on every iteration from
    // the second on).  First the block ends the iteration before met: level m's row was t - 1 - m, and its count
    // goes to that row's block row before the level counts on.  (MASK_UNI: uniform branches, every lane is here and
    // flushes into one block row, so the lanes of a block column add up first.  MASK_LANE: the lanes come one
    // segment at a time, and each adds its own count.)  Then this iteration's ends.
    __device__ __forceinline__ void row_phase(Tally& ty, int t) {
        if (ends != 0) {
#pragma unroll
            for (int m = 0; m < K; ++m)
                if ((ends >> m) & 1u) {
                    u32 rem;
                    const u32 brow = div_recip(gb + (u32)(t - 1 - m), block_rows, rows_recip, rem);
                    if (MASK == MASK_UNI && pre) ty.acc[m] = run_sum(ty.acc[m], run);
                    flush(ty, m, brow);
                }
        }
        const bool end = phase == block_rows - 1;
        phase = end ? 0u : phase + 1u;
        ends = ((ends << 1) | (end ? 1u : 0u)) & ((1u << K) - 1u);
    }

    // (BOUNDED) the loaded row: ghost rows and words hold the torus neighbour's cells
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) const {
        if (BOUNDED) em.apply(lo, hi, i);
    }
    // The (masked) output of level l is counted into acc[l].  Only owned rows are counted, and they are rows of the
    // board, global row gb + t: a count that is not zero at a block end belongs to that block (density_kernel.hip),
    // whatever gb + t and the phase are on other rows.
    __device__ __forceinline__ void level(Tally& ty, int l, u32& lo, u32& hi, int t) {
        if (BOUNDED) em.apply(lo, hi, t);
        if (l == 0 && maps) row_phase(ty, t);  // (maps: uniform)
        const u32 r = own.row(t);
        ty.acc[l] = (u32)__builtin_popcount(b3<kLutAnd3>(hi, own.own_hi, r)) + ty.acc[l];
        ty.acc[l] = (u32)__builtin_popcount(b3<kLutAnd3>(lo, own.own_lo, r)) + ty.acc[l];
    }
    // The end of the wave: every level has met the last owned row, so what is left (the block ends of the last
    // iteration included) belongs to the block row of that row.  Every lane is here: the lanes of a run with one
    // block (row and column) add up first.
    __device__ __forceinline__ void finish(Tally& ty) const {
        if (!maps) return;
        u32 rem;
        const u32 brow = div_recip(gb + (u32)own.Ao + own.ospan - 1u, block_rows, rows_recip, rem);
        if (pre) {
            const bool owns = (own.own_lo | own.own_hi) != 0 && own.ospan != 0;
            const u32 r = MASK == MASK_UNI ? run : runs_of(owns ? brow * grid_cols + bcol : kNoKey);
#pragma unroll
            for (int l = 0; l < K; ++l) ty.acc[l] = run_sum(ty.acc[l], r);
        }
#pragma unroll
        for (int l = 0; l < K; ++l) flush(ty, l, brow);
    }
};

// step_envelope's kernel argument: the envelope buffer, in the board's own layout (nullptr: touch nothing).
struct EnvelopeArgs {
    u64* env;
};

// The Tally of the envelope policy: the OR chains of the rows in flight.  nxt[l] is what level l - 1 made of its row
// in this row iteration, cur[l] what it made one iteration earlier: the OR of generations 1 .. l of the row level l
// outputs now.  Level 0 moves nxt to cur at the start of every iteration (renaming in the unrolled loop): cur[l] dies
// at level l and nxt[l] is born at level l - 1, so 2 (K - 1) values live across the iterations, and two more inside.
template <int K>
struct EnvelopeTally {
    u32 cur_lo[K], cur_hi[K], nxt_lo[K], nxt_hi[K];
    __device__ __forceinline__ EnvelopeTally() {
#pragma unroll
        for (int l = 0; l < K; ++l) cur_lo[l] = cur_hi[l] = nxt_lo[l] = nxt_hi[l] = 0;
    }
};

// step_envelope: the OR of a row's K outputs travels with the row through the levels; the last level ORs the owned
// cells of it into the envelope word that lies where the runner stores the row (envelope_kernel.hip).
template <int K, int MASK, bool BOUNDED>
struct EnvelopePolicy {
    static constexpr int kRowBarriers = 2;
    EdgeMask<MASK> em;  // BOUNDED
    OwnMask<MASK> own;
    unsigned long long* ep;  // the envelope word of the row level K - 1 outputs next (dereferenced by owning lanes only)
    const i64 pitch;
    const bool on;  // (uniform)
    using Tally = EnvelopeTally<K>;

    __device__ __forceinline__ EnvelopePolicy(const LaneDesc& d, int nrows, const StepParams& p, const TileArgs& ta,
                                              const EnvelopeArgs& ea)
        : pitch(p.pitch), on(ea.env != nullptr) {
        const bool stores = d.flags & LANE_STORE;  // (ahead of the masks: the prologue's order, PERFORMANCE.md section 23)
        if (BOUNDED) em.template init<K>(d, ta);
        own.template init<K>(stores, d, nrows, p, ta);
        // level K - 1 first outputs in row iteration 2K, row counter K: tile row row0, the runner's first store
        ep = reinterpret_cast<unsigned long long*>(ea.env) + ((i64)(d.row0 + p.R) * p.pitch + (d.col + 1));
    }

    // (BOUNDED) the loaded row: ghost rows and words hold the torus neighbour's cells
    __device__ __forceinline__ void input(u32& lo, u32& hi, int i) const {
        if (BOUNDED) em.apply(lo, hi, i);
    }
    // The (masked) output of level l joins the chain of its row; the last level's chain goes to the envelope.
    __device__ __forceinline__ void level(Tally& ty, int l, u32& lo, u32& hi, int t) {
        if (BOUNDED) em.apply(lo, hi, t);
        if (l == 0) {
#pragma unroll
            for (int m = 1; m < K; ++m) {
                ty.cur_lo[m] = ty.nxt_lo[m];
                ty.cur_hi[m] = ty.nxt_hi[m];
            }
        }
        const u32 e_lo = l == 0 ? lo : (ty.cur_lo[l] | lo), e_hi = l == 0 ? hi : (ty.cur_hi[l] | hi);
        if (l + 1 < K) {
            ty.nxt_lo[l + 1] = e_lo;
            ty.nxt_hi[l + 1] = e_hi;
            return;
        }
        if (!on) return;  // (uniform)
        const u32 r = own.row(t);
        const u32 m_lo = b3<kLutAnd3>(e_lo, own.own_lo, r), m_hi = b3<kLutAnd3>(e_hi, own.own_hi, r);
        // (a lane with nothing to add sends nothing: dead regions cost no envelope traffic)
        if ((m_lo | m_hi) != 0)
            (void)__hip_atomic_fetch_or(ep, ((unsigned long long)m_hi << 32) | (unsigned long long)m_lo, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
        ep += pitch;
    }
};

}  // namespace
}  // namespace hipk
}  // namespace gol
