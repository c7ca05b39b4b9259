// gol-mi355x: step_film<K, ROWS, BOUNDED> -- step_rule / step_rule_bounded that also stores the cells of a board
// window after every generation it computes, for gfx950 (CDNA4).
//
// A temporal-blocked pass keeps generations 1 .. K - 1 in registers only, so the cells of each generation can be
// kept nowhere but here.  Each level's output is already in two VGPRs (the word's even and odd cells); a lane whose
// word is a word of the window stores them, masked to the cells it owns, into the frame of that level:
//     frames[l * slot_words + frame_row * fw + frame_word] = {lo & own_lo, hi & own_hi}        (one global store)
// A frame (gol/film.hpp) is rows x fw board words in the split word format, fw the distinct board words the window's
// columns touch; the host takes the window's cells out of the words.  Nothing is accumulated: the policy has no
// tally and no finish, and a wave that misses the window pays the row test of every level and stores nothing.
//
// The kernel is the streaming wave of rule_runner.hpp (the gates, the level loop, the runner, the edge masks, the
// ownership masks and the choice between scalar and per-lane row tests) with the store as its policy.  Plans,
// StepParams, board loads and board stores are step_rule's.
//
// Which words are stored.  The lane test is formed once: the lane owns a word of the tile (OwnMask: a store lane,
// 0 <= col < nw), and the word's place in a frame row, (gword0 + col - w0) mod gwords, is below fw.  The row test is
// made per level: the row is owned (OwnMask::row, so it is a row of the tile and of the board) and its distance from
// the window's first row, (g - r0) mod H, is below rows; that distance is the frame row.  In a MASK_UNI wave the row
// tests and the frame row's address are scalar, in a MASK_LANE wave per lane.  The ownership argument of
// census_kernel.hip carries over: halo lanes, a segment's 2K extra rows, extension rows and ghost words are computed
// and never stored, outputs skipped while the pipeline fills are never owned rows, the interior and the bands of a
// split pass own disjoint words.  So every word of a frame is written by exactly one lane of one rank, no trash slot
// is needed and the stores need no atomics.  The address is the frames pointer (uniform) plus a 32-bit word index:
// the launcher refuses a pass whose K frames reach 2^31 bytes and one whose frames do not fit what the caller owns.
//
// frames == nullptr skips the stores (uniformly): the engine's init-time timing launches.
//
// Depths K = 1 .. 8, both row modes, both boundaries; registers: docs/PERFORMANCE.md section 25.
#include "rule_launch.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_film(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                  const LaneDesc* __restrict__ plan, StepParams p,
                                                                  RuleMasks rm, TileArgs ta, FilmArgs fa) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, FilmPolicy<K, MASK_UNI, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, fa);
        w.run();
    } else {
        RuleRunner<K, ROWS, FilmPolicy<K, MASK_LANE, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, fa);
        w.run();
    }
}

const void* film_kernel_of(Nbhd nbhd, int k, u32 flags, bool bounded) {
    if (nbhd != Nbhd::Moore) return nbhd_film_kernel(nbhd, k, flags, bounded);
    return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
        return bounded ? (const void*)step_film<K(), ROWS(), true> : (const void*)step_film<K(), ROWS(), false>;
    });
}

}  // namespace

int max_film_depth(Nbhd) { return kMaxRuleDepth; }

int film_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd) {
    return blocks_per_cu(film_kernel_of(nbhd, k, flags, bounded));
}

void launch_step_film(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                      const LaneDesc* plan, i64 n_waves, const StepParams& p, const FilmWindow& win, u64* frames,
                      i64 frames_words, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_film has no seam-reading variant (sub-tiles do not run film mode)");
    check_rule_masks("step_film", rule);
    check_place("step_film", place);
    check_tile_cols("step_film", tile_cols, p);
    // the frame stores: the window lies on the board, and the pass's k frames inside what the caller owns
    const i64 gwords = ceil_div(place.cols, 64);
    if (place.rows >= ((i64)1 << 30) || win.rows < 1 || win.rows > place.rows || win.fw < 1 || win.fw > gwords || win.r0 < 0 ||
        win.r0 >= place.rows || win.w0 < 0 || win.w0 >= gwords)
        throw Error(strprintf("step_film: a window of %lld rows x %lld words at row %lld, word %lld does not lie on the %lld x %lld board",
                              (long long)win.rows, (long long)win.fw, (long long)win.r0, (long long)win.w0, (long long)place.rows,
                              (long long)place.cols));
    const i64 slot = win.rows * win.fw;
    if (k < 1 || slot * 8 > (((i64)1 << 31) - 1) / k)
        throw Error(strprintf("step_film: %d frames of %lld words reach 2^31 bytes (the stores index with 32 bits)", k, (long long)slot));
    if (frames && frames_words < (i64)k * slot)
        throw Error(strprintf("step_film: %d frames of %lld words do not fit the %lld words left in the frame buffer", k,
                              (long long)slot, (long long)frames_words));
    const void* f = film_kernel_of(rule.nbhd, k, p.flags, bounded);
    if (!f) throw Error(strprintf("no film kernel instantiated for depth %d (1..%d)", k, kMaxRuleDepth));
    const FilmArgs fa{reinterpret_cast<uint2*>(frames), (u32)slot, (u32)win.rows, (u32)win.fw, (i32)win.r0, (i32)win.w0};
    launch_generic("film", f, rule, src, dst, plan, n_waves, p, s, tile_args(&place, tile_cols, p), fa);
}

}  // namespace hipk
}  // namespace gol
