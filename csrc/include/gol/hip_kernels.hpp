// gol-mi355x: host API of the hand-written gfx950 kernels (implemented in src/hip/*.hip).
//
// Kernel inventory (reference has one kernel, gol_kernel, gol-with-cuda.cu:189-262):
//   step_temporal<K>  — K generations of B3/S23 per pass over a bit-packed tile: wave64 column
//                       streaming, bit-sliced v_bitop3/v_alignbit adders, DPP wave_shr/shl lane
//                       exchange, K-deep register pipeline (temporal blocking), periodic wrap by
//                       load addressing.  Replaces gol_kernel + the per-generation sync/swap.
//   The four generic-rule kernels share one streaming wave (rule_runner.hpp: the rule gates, the level loop, the
//   runner, the edge and ownership masks) and one set of host-side checks (rule_launch.hpp); each adds a policy:
//   step_rule<K>      — step_temporal's streaming wave with a generic finish: any B0-free life-like rule
//                       B.../S... from two run-time masks (rule_kernel.hip; K = 1..8).
//   step_rule_bounded<K> — step_rule on a bounded board (dead cells beyond the global edges): the loaded row and
//                       every level masked to the board's cells (rule_bounded_kernel.hip; K = 1..8).
//   step_census<K>    — step_rule / step_rule_bounded that also counts the tile's live cells after every generation
//                       of the pass: a masked v_bcnt per level, K atomics per wave (census_kernel.hip; K = 1..8).
//   step_signature<K> — step_census that also hashes the tile after every generation of the pass: the linear,
//                       position-keyed board signature, two multiplies and two 64-bit multiply-adds per word and
//                       level (signature_kernel.hip; K = 1..8; with k_signature and k_board_diff).
//   Under a von Neumann or hexagonal rule (Rule::nbhd) the launchers of these four dispatch to the same streaming
//   wave with that neighbourhood's gates (nbhd_gates.hpp; instantiated in nbhd_rule_kernel.hip, nbhd_bounded_kernel.hip,
//   nbhd_census_kernel.hip, nbhd_signature_kernel.hip; K = 1..8): the depth and occupancy queries below take the
//   neighbourhood for that reason.
//   step_gen<K, M>    — Generations rules (B/S/C): step_rule / step_rule_bounded on the live plane with the dying
//                       cells' decay counter, M more bit planes, carried through the levels (generations_kernel.hip;
//                       K = 1 .. max_generations_depth(C); with k_state_counts and k_settle_decay in aux_kernels.hip).
//   step_ltl<R>       — Larger than Life rules (range R = 1 .. 7, the box neighbourhood, count intervals): one generation
//                       per pass on the same streaming wave, a bit-sliced (2R+1)^2 box sum from shifted copies, a ring
//                       of horizontal sums and a running column sum, four bit-sliced threshold compares (ltl_kernel.hip).
//   step_soups<M>     — soup batches (gol/soups.hpp), beside the engine: many independent 64 M x 64 M tori per launch, one
//                       wave64 per soup with the board in registers, settled inside the kernel (soup_kernel.hip; its host
//                       API is src/hip/soup_kernel.hpp).
//   step_lds          — single-generation LDS-tiled variant (tile + ghost words staged in LDS);
//                       kept as a measured alternative (GOL_KERNEL=lds).
//   fill_ghost_cols   — x-periodic ghost words for widths that are not a multiple of 64.
//   fill_ghost_rows   — y-periodic ghost rows for a tile shorter than the halo depth.
//   init_fill/set_cells — device-side pattern init (reference: host loops over managed memory).
//   copy_regions      — batched strided copies: 2-D halo pack/unpack and self-neighbour copies.
//   reduce_board      — population + decomposition-invariant fingerprint.
//   window_bytes / density / stamp — views of the live board and pattern stamping (view_kernels.hip).
//   match / match_positions — template matching on the live board and on soup batches (match_kernel.hip).
//   cc_init / cc_merge / cc_flatten / cc_roots / cc_stats / cc_hash / cc_labels — connected components of the live
//                       board and of soup batches: a lock-free union-find over runs of ones (components_kernel.hip).
//   naive_byte_step   — byte-per-cell, thread-per-cell yardstick of the reference's algorithm class
//                       (no printf), used only by the benchmark for comparison.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "gol/components.hpp"
#include "gol/density_film.hpp"
#include "gol/geometry.hpp"
#include "gol/match.hpp"
#include "gol/plan.hpp"
#include "gol/rule.hpp"

namespace gol {
namespace hipk {

enum : u32 {
    STEP_WRAP_X = 1u << 0,  // LDS kernel: tile is its own E/W neighbour (w % 64 == 0); the temporal
                            // kernel gets x-wrap from its plan (build_plan(..., xwrap = true))
    STEP_WRAP_Y = 1u << 1,  // tile is its own N/S neighbour: rows are read modulo h, no ghost rows
    STEP_TILE_L2 = 1u << 4, // tile kernel: two generations per LDS pass (half the barriers)
    STEP_TILE_L4 = 1u << 6, // tile kernel: four generations per LDS pass
    STEP_TILE_INPLACE = 1u << 7,  // tile kernel: one tile buffer updated in place (twice the rows)
    STEP_TILE_FOLD = 1u << 8,     // tile kernel: 32-lane tiles folded in half (fold plans, plan.hpp)
    STEP_SEAM = 1u << 5,    // temporal kernel: rows < 0 are read from StepParams::above, rows >= h
                            // from StepParams::below (sub-tile first pass: the other half's edges)
};

// Rows the HIP engine allocates past the bottom halo: the temporal kernel's 3-row prefetch overrun
// + the trash row its halo lanes store into (and the tile kernel's over-read slack).
constexpr int kSlackRows = 32;

struct StepParams {
    i64 pitch;
    i32 h;
    i32 nw;
    i32 R;
    u32 flags;
    // STEP_SEAM: row r < 0 of the source is at above + r * pitch, row r >= h at below + (r - h) * pitch
    // (word c at + c + 1, like the source buffer's rows)
    const u64* above = nullptr;
    const u64* below = nullptr;
    // Where lanes that store nothing (halo / idle lanes) write instead: kTrashWaves x 64 words, one
    // word per (wave mod kTrashWaves, lane).  Filled in by the launch functions (ensure_trash).
    u64* trash = nullptr;
};
constexpr int kTrashWaves = 1024;
// Allocate the current device's trash buffer (call once per device before any launch or capture;
// thread safe).
void ensure_trash();
u64* trash_of_current_device();  // (throws when ensure_trash has not run on this device)

// Supported temporal depths (template instantiations).
bool step_depth_supported(int k);
// Resident 256-thread workgroups per CU of step_temporal<k> for the given STEP_* flags.
int step_blocks_per_cu(int k, u32 flags);
int max_step_depth();
// Launch K generations: src -> dst over the waves of `plan` (n_waves * 64 LaneDescs in device memory).
void launch_step(int k, const u64* src, u64* dst, const LaneDesc* plan, i64 n_waves, const StepParams& p,
                 hipStream_t s);
// step_rule<K> (rule_kernel.hip): K generations of `rule` over the waves of `plan`, the same plans and
// StepParams as launch_step (STEP_SEAM excepted: it has no seam-reading variant).  It and the three kernels
// below read and write exactly the rows and words step_temporal<K> does for the same plan (rule_runner.hpp
// states the invariant once for all four).  Depths 1 .. max_rule_depth().
bool rule_depth_supported(int k, Nbhd nbhd = Nbhd::Moore);
int max_rule_depth(Nbhd nbhd = Nbhd::Moore);
int rule_blocks_per_cu(int k, u32 flags, Nbhd nbhd = Nbhd::Moore);
void launch_step_rule(int k, const Rule& rule, const u64* src, u64* dst, const LaneDesc* plan, i64 n_waves,
                      const StepParams& p, hipStream_t s);
// step_rule_bounded<K> (rule_bounded_kernel.hip): step_rule on a bounded board (Boundary::Dead).  Cells outside
// the global board are dead at the input and at every level of the pass.  Same plans (built without x-wrap, so
// a halo lane's column tells that it is outside), same StepParams, same rows and words read and written.
struct BoardEdges {
    i64 row0 = 0;   // global row of tile row 0
    i64 rows = 0;   // rows of the global board
    i64 word0 = 0;  // global word index of tile word 0
    i64 cols = 0;   // columns of the global board
};
int rule_bounded_blocks_per_cu(int k, u32 flags, Nbhd nbhd = Nbhd::Moore);
void launch_step_rule_bounded(int k, const Rule& rule, const BoardEdges& edges, const u64* src, u64* dst,
                              const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s);
// step_census<K> (census_kernel.hip): step_rule (edges == nullptr: the torus) or step_rule_bounded (edges) that also
// adds the live cells of the tile after generation g + 1 of the pass's k to the slot at counts + g * kCensusSlotWords
// (device memory, 64-bit atomics; nullptr: count nothing).  A slot is kCensusStripes partial sums kCensusStripeWords
// words apart (a 128-byte line each); the generation's count is their sum.  Every cell of the tile (tile_cols
// columns, p.h rows) is counted once per generation over the launches whose plans partition a pass's output
// region.  Same plans, StepParams, rows and words read and written, and the same argument checks, as
// launch_step_rule_bounded.  Depths 1 .. max_census_depth().
constexpr int kCensusStripes = 16, kCensusStripeWords = 16;
constexpr int kCensusSlotWords = kCensusStripes * kCensusStripeWords;  // u64 words from one generation's slot to the next
int max_census_depth(Nbhd nbhd = Nbhd::Moore);
int census_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd = Nbhd::Moore);
void launch_step_census(int k, const Rule& rule, const BoardEdges* edges, i64 tile_cols, const u64* src, u64* dst,
                        const LaneDesc* plan, i64 n_waves, const StepParams& p, u64* counts, hipStream_t s);
// step_signature<K> (signature_kernel.hip): step_census that also adds each generation's share of the board
// signature (gol/signature.hpp).  `place` is the tile's place on the board (always needed: the keys are global
// coordinates); `bounded` selects the dead-edge variant.  Generation g + 1 of the pass's k goes to the slot at
// slots + g * kSigSlotWords: kSigStripes partial counts kSigStripeWords words apart, then, kSigSigOffset words on,
// as many partial signatures (a 128-byte line each; the host adds them up, wrapping).  nullptr: record nothing.
// Plans, StepParams, rows and words read and written, and the argument checks, as launch_step_census.
// Depths 1 .. max_signature_depth().
constexpr int kSigStripes = 16, kSigStripeWords = 16;
constexpr int kSigSigOffset = kSigStripes * kSigStripeWords;  // u64 words from a slot's counts to its signatures
constexpr int kSigSlotWords = 2 * kSigSigOffset;              // u64 words from one generation's slot to the next
int max_signature_depth(Nbhd nbhd = Nbhd::Moore);
int signature_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd = Nbhd::Moore);
void launch_step_signature(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src,
                           u64* dst, const LaneDesc* plan, i64 n_waves, const StepParams& p, u64* slots, hipStream_t s);
// step_film<K> (film_kernel.hip): step_rule / step_rule_bounded that also stores the words of a board window after
// every generation of the pass.  `win` is the window in board rows and board words (gol/film.hpp: FilmGeo's r0,
// rows, w0, fw); the frame of generation g + 1 of the pass's k is the rows x fw words at frames + g * rows * fw
// (device memory, zeroed by the caller; nullptr: store nothing), of which this launch writes the words its plan's
// store lanes own, each exactly once.  frames_words: the words the caller owns from `frames` on; a pass that would
// store past them, or whose k frames reach 2^31 bytes, is refused before the launch.  Plans, StepParams, rows and
// words of the board read and written, and the argument checks, as launch_step_signature.  Depths 1 .. max_film_depth().
struct FilmWindow {
    i64 r0 = 0, rows = 0;  // board row of frame row 0, frame rows
    i64 w0 = 0, fw = 0;    // board word of frame word 0, words per frame row
};
int max_film_depth(Nbhd nbhd = Nbhd::Moore);
int film_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd = Nbhd::Moore);
void launch_step_film(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                      const LaneDesc* plan, i64 n_waves, const StepParams& p, const FilmWindow& win, u64* frames,
                      i64 frames_words, hipStream_t s);
// step_density<K> (density_kernel.hip): step_rule / step_rule_bounded that also counts the live cells of every block
// of the global board after every generation of the pass.  `grid` is the block shape and the grid
// (gol/density_film.hpp: DensityGeo, with blocks no larger than the board); the map of generation g + 1 of the pass's k is the grid_rows x grid_cols u32 at
// maps + g * slot words, slot = ceil(grid_rows * grid_cols / 2) (device memory, zeroed by the caller; nullptr: count
// nothing), to which this launch adds the cells its plan's store lanes own, each exactly once.  maps_words: the
// words the caller owns from `maps` on; a pass whose k maps do not fit them is refused before the launch.  Plans,
// StepParams, rows and words of the board read and written, and the argument checks, as launch_step_signature.
// Depths 1 .. max_density_depth().
int max_density_depth(Nbhd nbhd = Nbhd::Moore);
int density_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd = Nbhd::Moore);
void launch_step_density(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                         const LaneDesc* plan, i64 n_waves, const StepParams& p, const DensityGeo& grid, u64* maps,
                         i64 maps_words, hipStream_t s);
// step_envelope<K> (envelope_kernel.hip): step_rule / step_rule_bounded that also ORs every generation of the pass
// into the envelope.  `env` is a buffer in the board's own layout (the allocation of src and dst: same pitch, halo
// and slack rows; device memory; nullptr: touch nothing): after the launch, the envelope word at the offset of a
// word this launch's store lanes own also holds every cell of that word alive after generation 1 .. k of the pass;
// no other word of env is read or written.  Plans, StepParams, rows and words of the board read and written, and the
// argument checks, as launch_step_film.  Depths 1 .. max_envelope_depth().
int max_envelope_depth(Nbhd nbhd = Nbhd::Moore);
int envelope_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd = Nbhd::Moore);
void launch_step_envelope(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                          u64* env, const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s);
// step_gen<K, M> (generations_kernel.hip): K generations of a Generations rule (rule.states = C in 3 .. 9, Moore).  src
// and dst are boards of 1 + M planes in one layout, plane_stride words apart, M = rule.decay_planes(): plane 0 the live
// cells, which the kernel steps as step_rule / step_rule_bounded step a board, planes 1 .. M the decay counter of the
// dying cells.  In every plane it writes exactly the rows and words launch_step_rule writes in a board for the same plan,
// and reads the ones it reads, or at most three rows past a segment's last input row (within the slack rows the
// runner's prefetch requires); board_words is what the caller allocated per plane (the board, its halo and slack rows),
// and a plane_stride below it is refused.  `place`, `bounded`, tile_cols and the other argument checks as
// launch_step_envelope.  Depths 1 .. max_generations_depth(C).
int max_generations_depth(int states);
int generations_blocks_per_cu(int k, u32 flags, bool bounded, int states);
void launch_step_gen(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                     i64 plane_stride, i64 board_words, const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s);
// step_ltl<R, BOUNDED, MASK> (ltl_kernel.hip): one generation of a Larger than Life rule (rule.range = R in 1 .. 7, the
// box neighbourhood).  The plan is that of a pass of depth R (the generation's dependency cone: build_plan and
// validate_plan with k = R), p.R >= R, p.h >= 2R + 1 and STEP_WRAP_Y (one rank: rows are read modulo h; a bounded board
// masks the rows that wrap).  For the same plan it reads and writes no row or word step_temporal<R> would not: the
// same words written, and no row read past a segment's last input row.  `place` and `bounded` as launch_step_envelope.
int ltl_blocks_per_cu(int range, bool bounded);
void launch_step_ltl(const Rule& rule, const BoardEdges& place, bool bounded, const u64* src, u64* dst, const LaneDesc* plan,
                     i64 n_waves, const StepParams& p, hipStream_t s);
// Generations rules (aux_kernels.hip).  state_counts: the tile's own cells in state s, s = 0 .. C - 1, added to the kCensusStripes
// partial sums of slot s of `out` (the census's layout: C slots of kCensusSlotWords words, zeroed by the caller).
// settle_decay: every decay plane ANDed with the complement of the live plane over the tile's own words.
void launch_state_counts(const u64* buf, const Layout& L, i64 plane_stride, const Rule& rule, u64* out, hipStream_t s);
void launch_settle_decay(u64* buf, const Layout& L, i64 plane_stride, const Rule& rule, hipStream_t s);
// env = (reset ? 0 : env) | the tile's own cells of `board` (aux_kernels.hip; both buffers in layout L).
void launch_envelope_merge(u64* env, const u64* board, const Layout& L, bool reset, hipStream_t s);
// out[0] += the signature of the tile in `buf` at (grow0, gword0) (wrapping; out zeroed by the caller).
void launch_signature(const u64* buf, const Layout& L, i64 grow0, i64 gword0, u64* out, hipStream_t s);
// out[0] += the number of cells of the tile that differ between boards a and b (one layout; out zeroed by the caller).
void launch_board_diff(const u64* a, const u64* b, const Layout& L, u64* out, hipStream_t s);
// LDS-resident temporal kernel (step_tile): one workgroup of `nw_per_wg` (4, 8, 16) waves per plan
// wave; `rows` = the plan's rows per chunk (<= tile_max_rows(k), the 160 KiB LDS limit).
constexpr size_t kMaxLdsBytes = 160 * 1024;
// Least chunk height of a folded-tile plan (STEP_TILE_FOLD): its segments are >= 14 rows tall.
constexpr int kFoldMinRows = 28;
i64 tile_max_rows(int k, int nw_per_wg, u32 flags);
int tile_blocks_per_cu(int nw_per_wg, i64 rows, int k, u32 flags);
void launch_step_tile(int nw_per_wg, int k, const u64* src, u64* dst, const LaneDesc* plan, i64 n_tiles, i64 rows,
                      const StepParams& p, hipStream_t s);
// step_resident (resident_kernel.hip): a run of G generations in one launch, one workgroup of `nw`
// (8, 16) waves per tile of `plan` (one tile per CU, all co-resident), each wave holding B rows of
// the tile's extended rows (nrows + 2 kmax) in registers; S supersteps (odd) of <= kmax generations,
// between which tiles exchange halos through HBM with their neighbour tiles (CSR nbr_off / nbr,
// plan.hpp resident_neighbours) and per-tile counters.  The result is in dst.
struct ResidentParams {
    i64 pitch;
    i32 h;
    i32 R;
    i32 G;       // generations of this launch
    i32 S;       // supersteps (odd), of G / S or G / S + 1 generations
    i32 kmax;    // halo rows of the tiles: >= ceil(G / S)
    u64 timeout_ticks;  // bound of every neighbour wait, in s_memrealtime ticks (100 MHz)
};
// Instantiated: 16 waves x B in {2, 3, 4, 5, 6, 8} and 8 waves x B in {3, 4, 5, 6, 8, 10, 12, 16}, the tile its own
// N/S neighbour (wrapy); anything else throws "no kernel for ...".
int resident_band_rows(int rows_needed);  // supported band height >= rows_needed (0: none)
int resident_blocks_per_cu(int nw, int B, bool wrapy);
void launch_step_resident(int nw, int B, bool wrapy, u64* src, u64* dst, const LaneDesc* plan, i64 n_tiles,
                          const u32* nbr_off, const u32* nbr, u32* counters, u32* status, const ResidentParams& rp,
                          hipStream_t s);
// step_pipe (pipe_kernel.hip): K = nw x L generations per launch, one workgroup of `nw` (4, 8, 12,
// 16) waves per plan wave (a segment of the plan, as step_tile), wave w computing levels
// w L + 1 .. (w + 1) L of the whole segment and handing its rows to wave w + 1 through an LDS ring.
size_t pipe_lds_bytes(int nw);
bool pipe_supported(int nw, int L);
int pipe_blocks_per_cu(int nw, int L, bool wrapy);
// True (and cleared) when a step_pipe wait timed out since the last call: the board is invalid.
bool pipe_fault();
#ifdef GOL_PIPE_STAMPS
// Diagnostic build: per-wave wait stamps of the last step_pipe launch (pipe_kernel.hip g_pipe_stamps)
std::vector<u64> pipe_stamps(size_t waves);
#endif
void launch_step_pipe(int nw, int L, const u64* src, u64* dst, const LaneDesc* plan, i64 n_tiles, const StepParams& p,
                      hipStream_t s);
// Single-generation LDS-tiled kernel over output rows [r0, r1) (all words).
void launch_step_lds(const u64* src, u64* dst, const Layout& L, i64 r0, i64 r1, u32 flags, hipStream_t s);

void launch_fill_ghost_cols(u64* buf, const Layout& L, i64 r_lo, i64 r_hi, hipStream_t s);
void launch_fill_ghost_rows(u64* buf, const Layout& L, hipStream_t s);

struct InitParams {
    i64 row0;     // global row of tile row 0
    i64 gword0;   // global word index of tile word 0
    i64 gwords;   // words per global row
    u64 seed;
    int fill;     // 0 zero, 1 ones, 2 random
};
void launch_init_fill(u64* buf, const Layout& L, const InitParams& ip, hipStream_t s);
// cells: device array of (row, col) tile coordinates
void launch_set_cells(u64* buf, const Layout& L, const i64* cells, i64 n, hipStream_t s);

struct CopyDesc {
    const u64* src;
    u64* dst;
    i64 src_stride;  // words between rows
    i64 dst_stride;
    i32 rows;
    i32 words;
};
void launch_copy_regions(const CopyDesc* descs, int n, i64 max_elems, hipStream_t s);

// out[0] += population, out[1] += fingerprint (wrapping sums); out must be zeroed by the caller.
void launch_reduce_board(const u64* buf, const Layout& L, i64 grow0, i64 gword0, i64 gwords, u64* out,
                         hipStream_t s);

// ----- views and stamping (view_kernels.hip) -----
// A rectangle of cells in tile coordinates, inside the tile (the launchers check it).
struct ViewRect {
    i64 tr, tc;  // first row / column
    i64 rows, cols;
};
// window_bytes: the rectangle's cells as 0/1 bytes, dst[r * cols + c] (dst 16-byte aligned).
void launch_window_bytes(const u64* buf, const Layout& L, const ViewRect& rc, u8* dst, hipStream_t s);
// density: counts[bi * grid_cols + bj] += live cells of the tile in block (bi, bj) of the global board, blocks of
// block_rows rows x block_words words; (row0, gword0) is the tile's place on the board.
void launch_density(const u64* buf, const Layout& L, i64 row0, i64 gword0, i64 block_rows, i64 block_words,
                    i64 grid_cols, u32* counts, hipStream_t s);
// stamp: the rectangle's cells combined with the pattern's (natural-order words in device memory, pnw per row),
// whose cell (pr0, pc0) lands on the rectangle's first cell; mode 0 or, 1 replace, 2 xor, 3 clear.
void launch_stamp(u64* buf, const Layout& L, const ViewRect& rc, const u64* pat, i64 pnw, i64 pr0, i64 pc0, int mode,
                  hipStream_t s);

// ----- pattern matching (match_kernel.hip; gol/match.hpp) -----
// Where the boards are: board b's word c of row r is at base + b * batch_stride + r * pitch + c (words), rows 0 .. h - 1,
// words 0 .. nw - 1 = ceil(w / 64); nothing else is read.  The engine's board: match_geo(L, torus), i.e. base = R * pitch + 1,
// one board.  A soup batch: base 0, pitch = nw, batch_stride = h * nw.
struct MatchGeo {
    i64 base = 0, pitch = 0, batch_stride = 0;
    i64 w = 0;
    i32 h = 0, nw = 0;
    i32 torus = 1;  // 1: coordinates wrap; 0: cells outside the board are dead
    i32 batch = 1;
};
MatchGeo match_geo(const Layout& L, bool torus);
// k_match: for every word of every board the 64-bit bitmap of the cells at which `t` matches, in the board's split
// format, stored at the word's own offset in `bitmap` (a buffer addressed like the boards; nullptr: not stored; or_into:
// ORed into what is there), and the number of matches added to count32[b] (one u32 per board) or to count64[0] (one
// board only); the caller zeroes the counters.  Validates the template against the board before the launch.
void launch_match(const u64* board, const MatchGeo& g, const MatchTemplate& t, u64* bitmap, bool or_into, u32* count32,
                  u64* count64, hipStream_t s);
// k_match_positions: the set bits of board 0's bitmap as (row, col) pairs of i32 in no particular order: the first `cap`
// to arrive are stored at out, and cursor[0] (zeroed by the caller) ends as the number of set bits.
void launch_match_positions(const u64* bitmap, const MatchGeo& g, i32* out, i64 cap, u64* cursor, hipStream_t s);

// ----- connected components (components_kernel.hip; gol/components.hpp) -----
// The boards are addressed by a MatchGeo.  parent: cc_parent_bytes(g) = 4 bytes per cell of every board, uninitialised
// (only the slots of run heads are used).  All launchers refuse batch * h * w >= 2^31.  The order of a call:
//   launch_cc_init, launch_cc_merge                                     the forest of the runs;
//   launch_cc_roots with rec = nullptr                                  count[0] (and per_board[b]) alone; or
//   launch_cc_flatten, then launch_cc_labels                            the label tensor of one board; or
//   launch_cc_flatten, launch_cc_roots, launch_cc_stats, launch_cc_hash the records: rec (cap CcRecords) and sums (cap x 8
//                                                                       u64, nullptr: no hashes) need no clearing, the
//                                                                       counters do.
// Objects beyond the first cap to draw an id are counted and get no record.  wave_reduce = false leaves out the
// reduction across a wave whose words all lie in one object (a measurement switch; the results are the same).
size_t cc_parent_bytes(const MatchGeo& g);
void launch_cc_init(const u64* board, const MatchGeo& g, i32* parent, hipStream_t s);
void launch_cc_merge(const u64* board, const MatchGeo& g, CcNeighbourhood nb, i32* parent, hipStream_t s);
void launch_cc_flatten(const u64* board, const MatchGeo& g, i32* parent, hipStream_t s);
void launch_cc_roots(const u64* board, const MatchGeo& g, i32* parent, u32* count, u32* per_board, CcRecord* rec, u64* sums,
                     i64 cap, hipStream_t s);
void launch_cc_stats(const u64* board, const MatchGeo& g, const i32* parent, CcRecord* rec, i64 cap, bool wave_reduce, hipStream_t s);
void launch_cc_hash(const u64* board, const MatchGeo& g, const i32* parent, const CcRecord* rec, u64* sums, i64 cap,
                    bool wave_reduce, hipStream_t s);
// (h, w) labels of board 0 in row-major order, i32 or i64 elements (16-byte stores where w % 4 == 0 and out is aligned)
void launch_cc_labels(const u64* board, const MatchGeo& g, const i32* parent, void* out, bool int64, hipStream_t s);
// The whole records call on one stream, shared by the engine and the soup batches: scratch is allocated here and freed
// before the return (see docs/PERFORMANCE.md, section 33), and only the counters and the records leave the device.
ComponentsResult run_components(const u64* board, const MatchGeo& g, CcNeighbourhood nb, i64 max_objects, bool hashes,
                                bool want_records, hipStream_t s);
// The label call (init, merge, flatten, labels) with the same scratch handling; synchronises s before it returns.
void run_component_labels(const u64* board, const MatchGeo& g, CcNeighbourhood nb, void* out, bool int64, hipStream_t s);
// Measurement switch for tools/measure_components.py: whether run_components() lets k_cc_stats and k_cc_hash reduce
// across a wave (the default).  Process-wide; the results do not depend on it.
void cc_set_wave_reduce(bool on);

// Yardstick: one byte per cell, one thread per cell, x-wrap + two ghost rows (reference class).
void launch_naive_byte_step(const u8* src, u8* dst, i64 w, i64 h, const u8* above, const u8* below, int threads,
                            hipStream_t s);

}  // namespace hipk
}  // namespace gol
