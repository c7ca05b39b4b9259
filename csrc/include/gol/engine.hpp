// gol-mi355x: the generation engine (superstep scheduler) — CPU and HIP backends.
//
// Reference loop (gol-main.c:93-116, gol-with-cuda.cu:264-284): for every generation, 2 Irecv +
// 2 Isend of one byte row, wait for the receives, launch gol_kernel, cudaDeviceSynchronize, swap.
//
// Engine loop: generations are grouped into supersteps of k <= R generations.  Per superstep:
//   1. halo refresh — exchange k-deep halos with the neighbours (canonical order, one transport call:
//      1-D: 2 contiguous full-pitch row blocks sent straight from / received straight into the board;
//      2-D: 8 packed regions incl. corners).  Self-neighbour directions need nothing: the kernel
//      wraps rows / columns by addressing.
//   2. compute — k generations in one pass of the temporal kernel.  With overlap, the interior
//      (rows that only need local data) runs on the compute stream while the exchange runs on the
//      comm stream; the boundary bands follow once the halo has landed.
//   3. swap (parity flip).
// On the HIP backend supersteps are captured into hipGraphs (pairs, so parity is preserved) and
// replayed; there is no host synchronisation inside run().
#pragma once

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "gol/cells.hpp"
#include "gol/components.hpp"
#include "gol/density_film.hpp"
#include "gol/film.hpp"
#include "gol/geometry.hpp"
#include "gol/match.hpp"
#include "gol/pattern.hpp"
#include "gol/plan.hpp"
#include "gol/rle.hpp"
#include "gol/rule.hpp"
#include "gol/transport.hpp"
#include "gol/watchdog.hpp"

namespace gol {

// Tile rows from which GOL_SUBTILES=auto uses two sub-tiles (measured: 32768^2 +3-5% per generation,
// 65536^2 equal, 16384^2 -3%; docs/PERFORMANCE.md).
constexpr i64 kSubtileMinRows = 24576;

struct EngineConfig {
    std::string backend = "cpu";      // cpu | hip
    int halo_depth = 0;               // R: generations per halo exchange (0 = auto: 8 on one rank,
                                      // 32 for 1-D multi-rank; clamped to the geometry)
    int kernel_depth = 0;             // K: generations per kernel pass (0 = auto; HIP)
    bool overlap = true;              // interior/boundary split with comm-stream exchange
    bool graph = true;                // hipGraph capture of superstep pairs
    bool compat = false;              // reference halo quirks (Q1/Q2), 1-D only, k = 1
    int device = -1;                  // HIP device (-1: current)
    i64 rows_per_wave = 0;            // plan segment height override (0 = auto)
    int waves_target = 0;             // plan wave-count target (0 = auto)
    int plan_xcds = 8;                // XCD-aware plan order (workgroup b runs on XCD b % n; 1 = off)
    std::string kernel = "auto";      // auto (timed at init) | temporal (register pipeline) |
                                      // tile (LDS-resident) | lds (1 gen, reference-class LDS tile) |
                                      // rule (the generic life-like-rule kernel, also for B3/S23)
    Rule rule;                        // the life-like rule (default B3/S23; GOL_RULE).  Any other rule runs
                                      // the generic paths: cpu::step_rows' bit-sliced count, step_rule on HIP
    Boundary boundary = Boundary::Torus;  // Torus (the reference) | Dead: cells outside the global board are
                                      // dead in every generation (GOL_BOUNDARY).  The torus machinery (ghost
                                      // fills, exchanges with the wrap-around neighbour) keeps running; what it
                                      // delivers across a global edge is masked away.  HIP: step_rule_bounded
    bool census = false;              // census mode (GOL_CENSUS): every generation run() computes also yields the
                                      // global live-cell count of that generation (Engine::census).  HIP: the
                                      // census kernel step_census runs every pass, for every rule and boundary
    bool signature = false;           // signature mode (GOL_SIGNATURE): every generation run() computes also yields
                                      // the board signature (gol/signature.hpp) and the population of that
                                      // generation (Engine::signatures).  HIP: step_signature runs every pass.
                                      // Not together with census (signature mode records the population too)
    FilmRect film;                    // film mode (GOL_FILM=r0,c0,rows,cols): every generation run() computes also yields
                                      // the cells of that window of the global board, window()'s coordinates and checks
                                      // (Engine::film).  HIP: step_film stores them inside every pass.  Not together with
                                      // census or signature
    DensityBlocks density_film;       // density-film mode (GOL_DENSITY_FILM=block_rows[,block_cols]): every generation run()
                                      // computes also yields the density(block_rows, block_cols) grid of the global
                                      // board (Engine::density_film).  HIP: step_density counts it inside every pass.
                                      // Not together with census, signature or film
    bool envelope = false;            // envelope mode (GOL_ENVELOPE): the engine keeps the OR of every generation of the
                                      // board since the last reset, one bit per cell (Engine::envelope_*).  HIP: a third
                                      // board-sized buffer, and step_envelope ORs into it inside every pass.  Not
                                      // together with census, signature, film or density_film
    int tile_waves = 8;               // tile kernel: waves per workgroup (4, 8, 16)
    bool tune_tile_waves = true;      // GOL_KERNEL=auto may also try 8 waves (false: GOL_TILE_WAVES set)
    std::string transport = "auto";   // auto | device | host  (host = stage halos through host memory)
    bool profile = false;             // per-phase event timing
    int graph_supersteps = 0;         // supersteps per captured graph (0 = auto, even)
    int subtiles = -1;                // HIP, 1-D: two sub-tiles per rank on two streams (GOL_SUBTILES:
                                      // 2 on, 0 off, -1 auto = on for tiles of >= kSubtileMinRows rows)
    u64 run_hint = 0;                 // generations of the runs to come (CLI: iterations); the HIP
                                      // engine captures one graph covering them (<= 256 supersteps)
    int graph_rccl = -1;              // one-tile supersteps whose exchange is an RCCL group, captured in
                                      // hipGraphs (GOL_GRAPH_RCCL: 1 on, 0 off, -1 = a candidate of the
                                      // init-time schedule timing, "full+graph")
    int subtile_overlap = -1;         // sub-tiles with neighbours: half 0 starts its first pass (all but
                                      // its band next to the rank's north halo) while the exchange is in
                                      // flight (GOL_SUBTILE_OVERLAP: 1 on, 0 off, -1 = a candidate of the
                                      // init-time schedule timing, "subtiles+ov")
    int sub_occ = 2;                  // sub-tile plans: waves per SIMD each half is sized for (GOL_SUB_OCC;
                                      // 0 = the single-tile tuned occupancy)
    bool self_exchange = false;       // GOL_SELF_EXCHANGE: directions whose neighbour is this rank go
                                      // through the transport (peer == rank) instead of wrapping by
                                      // addressing: runs every halo path of the multi-GPU engine on
                                      // one rank (e.g. a 1-rank RCCL communicator)
    double watchdog_s = 0;            // abort the job after this long without progress (0 = off)
    bool force_split = false;         // run the interior/boundary edge schedule even without neighbours
    std::string sched = "auto";       // auto (timed at init) | split (overlap, with neighbours) | full
};

struct EngineStats {
    u64 generations = 0;
    u64 supersteps = 0;
    u64 exchanges = 0;
    u64 halo_bytes = 0;       // bytes sent by this rank
    u64 graph_launches = 0;
    int depth = 0;            // R (generations per halo exchange)
    int kernel_depth = 0;     // K (generations per kernel pass)
    int tile_waves = 0;       // HIP: workgroup size of the LDS tile kernel (waves)
    i64 plan_waves = 0;       // waves of the full-tile plan
    double lane_efficiency = 0;  // output words / (64 * input rows * waves) for the full plan
    // HIP: us per generation of the chosen schedule, timed at the end of init the way a hinted run
    // executes (same supersteps, graphs or eager launches, after a device barrier, from an idle GPU);
    // 0 when not measured
    double predicted_us_per_gen = 0;
    int predicted_gens = 0;     // generations of the timed supersteps behind it
    double t_exchange_ms = 0;  // profile only
    double t_compute_ms = 0;   // profile only
    std::string kernel;        // stencil kernel in use (HIP: temporal | tile | lds | rule@K | gen@K | ltl@1; CPU: cpu)
    std::string rule;          // the rule, canonical (B3/S23; a Generations rule: B2/S345/C4; LtL: R5,C0,M1,S34..58,B34..45,NM)
    int states = 2;            // its states: 2, or C of a Generations rule
    std::string boundary;      // torus | dead
    bool census = false;       // census mode
    bool signature = false;    // signature mode
    FilmRect film;             // film mode: the window (on = false: off)
    DensityBlocks density_film;  // density-film mode: the blocks (on = false: off)
    bool envelope = false;     // envelope mode
    u64 envelope_start = 0;    // envelope mode: the generation of the envelope's last reset
    std::string schedule;      // superstep schedule: local (no neighbours) | split | full
    std::string tuning;        // init-time measurements behind the auto choices (HIP)
    bool registered = false;   // HIP + RCCL: the boards are registered with the communicator (zero-copy halos)
    u64 view_bytes_d2h = 0;    // HIP: bytes window() copied from the device (this rank's cells of the windows)
    u64 match_launches = 0;    // matcher runs of match() and match_cells(), one per oriented template (HIP: k_match launches)
};

// How stamp() combines a pattern with the board.  Replace overwrites the pattern's bounding rectangle;
// Clear kills the cells where the pattern is live.
enum class StampMode : int { Or = 0, Replace, Xor, Clear };
StampMode parse_stamp_mode(const std::string& s);  // or | replace | xor | clear

class Engine {
   public:
    static std::unique_ptr<Engine> create(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t);
    virtual ~Engine() = default;

    void init(const PatternSpec& p);
    virtual void run(u64 generations);
    virtual void synchronize() = 0;
    // True when none of the engine's own GPU work is outstanding (non-blocking query; CPU: always).
    virtual bool gpu_idle() { return true; }

    // Local tile as dense masked words (h * nw), and the reverse (halos are refreshed).
    virtual std::vector<u64> tile_words() = 0;
    virtual void set_tile_words(const std::vector<u64>& dense) = 0;
    // (population, fingerprint) of the local tile.
    virtual std::pair<u64, u64> local_reduce() = 0;
    // Global values (collective over the transport).
    u64 population();
    u64 fingerprint();

    // ----- census (EngineConfig::census) -----
    // Collective: (start, counts), counts[i] the GLOBAL population at generation start + 1 + i, for every
    // generation run() has computed since the record was cleared: by init() (start 0), by a checkpoint restore
    // (start: the restored generation) or by census_clear() (start: the generation reached).  stamp() and
    // set_tile_words() leave it alone: the generation count runs on.  The same on every rank (the ranks' series
    // are summed over the control plane: gatherv to rank 0, broadcast).  Throws, before any communication, on an
    // engine that is not in census mode.
    std::pair<u64, std::vector<u64>> census();
    void census_clear();
    void census_restart(u64 generation);  // an empty record that starts at `generation` (load_checkpoint; both modes)

    // ----- signatures (EngineConfig::signature) -----
    // The board signature (gol/signature.hpp): a linear, position-keyed 64-bit hash of the global board, equal for
    // every decomposition.  signatures() is census() of signature mode: (start, signatures, populations), entry i
    // for generation start + 1 + i, with the same start / clear / restart rules (census_restart serves both modes)
    // and the same collective sum over the ranks (wrapping, for the signatures).
    struct SignatureSeries {
        u64 start = 0;
        std::vector<u64> signatures, populations;
    };
    SignatureSeries signatures();
    void signatures_clear();
    // Collective, any mode: the signature of the current board.
    u64 signature();
    // snapshot(): keep a copy of this rank's current board (a third tile-sized buffer, allocated on first use; throws
    // when the memory is not there).  snapshot_diff(): collective, the number of cells of the GLOBAL board that
    // differ between the current board and the snapshot; throws, before any communication, without a snapshot.
    void snapshot();
    u64 snapshot_diff();
    // run() keeps a record made inside the stepping kernel: per generation, or (envelope mode) one OR over them
    bool recording() const { return cfg_.census || cfg_.signature || cfg_.film.on || cfg_.density_film.on || cfg_.envelope; }

    // ----- Generations rules (EngineConfig::rule with states > 2; gol/rule.hpp) -----
    // The board is 1 + M planes in one layout: the live plane (state 1), which is the board every other call of this
    // class reads and writes (tile_words, population, density, fingerprint, signature, snapshot*, match, window, stamp),
    // and the M planes of the decay counter of the dying cells.  No cell is alive and dying; tail bits, ghost words
    // outside a bounded board and slack rows are zero in every plane.  One rank only.  init() and set_tile_words() zero
    // the decay planes; stamp() acts on the live plane and then clears the decay counter of every live cell (so a
    // stamped cell is alive, and `replace` and `clear` leave dying cells dying).  HIP: step_gen runs every pass.
    // The calls below throw on an engine whose rule has two states.
    int states() const { return (int)cfg_.rule.states; }
    bool generations() const { return cfg_.rule.generations(); }
    std::vector<u8> state_tile();                          // h x w bytes: the state 0 .. C-1 of every cell of the tile
    void set_state_tile(const std::vector<u8>& states);    // (every value checked to be < C before anything is written)
    std::vector<u8> state_window(i64 r0, i64 c0, i64 rows, i64 cols);  // window()'s coordinates and checks
    std::vector<u64> state_counts();                       // C counts: the cells of the board in each state
    // Throws, naming the call and the rule, under a Generations rule: what is not built for them in this version.
    void need_two_states(const char* what) const;
    // ----- Larger than Life rules (EngineConfig::rule with range > 0; gol/rule.hpp) -----
    // Two states on the ordinary board: every reader and writer of the board works unchanged.  One rank; a superstep is
    // one generation (stats.depth and stats.kernel_depth are 1) although the layout's halo depth is the rule's range, the
    // depth of the generation's dependency cone.  need_rule_code throws, naming the call and the rule, under such a rule:
    // checkpoints, which need Rule::code().
    bool ltl() const { return cfg_.rule.ltl(); }
    void need_rule_code(const char* what) const;

    // ----- envelope (EngineConfig::envelope) -----
    // E = board(start) | board(start + 1) | ... | board(generation()), cell by cell, with start the generation of the
    // last reset: init(), set_tile_words() (so a checkpoint restore too) and envelope_clear() make E the current board
    // and start the generation reached; stamp() is followed by E |= board.  Each rank keeps E for its own tile, in
    // the board's layout.  The readers are the board's readers run on E: envelope_tile_words() this rank's tile (no
    // communication), the others collective and the same on every rank.  All throw, before any communication, on an
    // engine that is not in envelope mode.
    u64 envelope_start() const;
    std::vector<u64> envelope_tile_words();
    std::vector<u8> envelope_window(i64 r0, i64 c0, i64 rows, i64 cols);
    std::vector<u32> envelope_density(i64 block_rows, i64 block_cols);
    u64 envelope_population();
    void envelope_clear();

    // ----- film (EngineConfig::film) -----
    // Collective: (start, n, frames): frame i, rows x cols 0/1 bytes at frames[i * rows * cols], is what
    // window(r0, c0, rows, cols) would return at generation start + 1 + i, for every generation run() has computed
    // since the record was cleared; the start, clear and restart rules are the census's (census_restart serves this
    // mode too).  The same on every rank: each rank records the words of the window it owns (gol/film.hpp), the ranks'
    // packed frames are summed over the control plane (disjoint bits) and unpacked on the host.  Throws, before any
    // communication, on an engine that is not in film mode.
    struct Film {
        u64 start = 0;
        size_t n = 0;
        std::vector<u8> frames;
    };
    Film film();
    void film_clear();
    // film() in two steps, for a caller that owns the bytes: film_frames() brings this rank's record to the host and
    // returns its frames (the same number on every rank; no communication); film_into() is the collective part and
    // unpacks them into out (n * rows * cols bytes, n as returned), several rows at a time; it returns start.
    size_t film_frames();
    u64 film_into(u8* out, size_t n);
    const FilmGeo& film_geo() const { return film_geo_; }

    // ----- density film (EngineConfig::density_film) -----
    // Collective: (start, n, maps): map i, grid_rows x grid_cols counts at maps[i * grid_rows * grid_cols], is what
    // density(block_rows, block_cols) would return at generation start + 1 + i, for every generation run() has
    // computed since the record was cleared; the start, clear and restart rules are the census's (census_restart
    // serves this mode too).  The same on every rank: each rank counts the cells it owns (gol/density_film.hpp) and
    // the ranks' maps are summed over the control plane, a few maps at a time.  Throws, before any communication, on
    // an engine that is not in density-film mode.
    struct DensityFilm {
        u64 start = 0;
        size_t n = 0;
        std::vector<u32> maps;
    };
    DensityFilm density_film();
    void density_film_clear();
    // density_film() in two steps, for a caller that owns the counts: density_film_frames() brings this rank's record
    // to the host and returns its maps (the same number on every rank; no communication); density_film_into() is the
    // collective part and writes the summed maps into out (n * grid_rows * grid_cols counts, n as returned); it
    // returns start.
    size_t density_film_frames();
    u64 density_film_into(u32* out, size_t n);
    const DensityGeo& density_geo() const { return density_geo_; }

    // ----- views and pattern stamping -----
    // Global board coordinates on the torus: a window or a pattern may start anywhere (r0, c0 are taken
    // modulo the board), cross the board's seams and any rank boundary; it is at most the board's size.
    // On a bounded board the rectangle must lie inside the board (0 <= r0, r0 + rows <= H, likewise columns).
    // The *_local virtuals do this rank's part, the wrappers below them are collective and return the
    // whole result on every rank (the parts travel over the control plane: gatherv to rank 0, broadcast).
    // Arguments are validated before any communication: a bad call throws on every rank, none hangs.
    //
    // This rank's cells of the window as 0/1 bytes at out[i * stride + j]; other ranks' cells are untouched.
    virtual void read_window_local(i64 r0, i64 c0, i64 rows, i64 cols, u8* out, i64 stride) = 0;
    // Adds the live-cell counts of this rank's cells into a ceil(H / block_rows) x ceil(W / block_cols) grid
    // over the global board (edge blocks are partial).  block_cols is a multiple of 64.
    virtual void density_local(i64 block_rows, i64 block_cols, u32* counts) = 0;
    // Combines this rank's cells of the pattern's rectangle at (r0, c0) with the board; ghosts and halos are
    // brought up to date as set_tile_words does.  Refused for a pattern larger than the board (it would
    // overlap itself) and in compat mode (its halos are frozen at generation 0).
    virtual void stamp_local(const RlePattern& p, i64 r0, i64 c0, StampMode mode) = 0;
    std::vector<u8> window(i64 r0, i64 c0, i64 rows, i64 cols);     // rows x cols bytes
    std::vector<u32> density(i64 block_rows, i64 block_cols);        // density_rows() x density_cols()
    void stamp(const RlePattern& p, i64 r0, i64 c0, StampMode mode);  // (no communication: every rank holds p)
    // The part of the wrapped global rectangle (r0, c0, rows, cols) inside the tile of geometry g: at most
    // four pieces (the rectangle is cut where it crosses the board's seams).
    struct Piece {
        i64 tr, tc;        // first row / column in tile coordinates
        i64 rows, cols;
        i64 wr, wc;        // the piece's offset inside the rectangle
    };
    static std::vector<Piece> pieces(const Geometry& g, i64 r0, i64 c0, i64 rows, i64 cols);
    // (on a bounded board the rectangle must lie inside the board: the overloads with r0, c0)
    void check_window(i64 rows, i64 cols) const;
    void check_window(i64 r0, i64 c0, i64 rows, i64 cols) const;
    void check_density(i64 block_rows, i64 block_cols) const;
    void check_stamp(const RlePattern& p) const;
    void check_stamp(const RlePattern& p, i64 r0, i64 c0) const;
    // ----- pattern matching (gol/match.hpp) -----
    // Where the oriented templates `ts` ((orientation id, template), MatchTemplate::orientations) match on the current
    // board, torus or bounded as the engine runs.  One rank only: more throw, naming the rank count, before anything is
    // launched (the neighbours' rows would be needed).  Every template is validated against the board first, and
    // max_hits < 1 is refused.  HIP: k_match writes a board-sized bitmap and a counter, k_match_positions compacts the
    // bitmap; only the counter and the positions leave the device.
    struct MatchResult {
        u64 count = 0;                 // matches over all the templates of `ts`; always exact
        std::vector<i32> positions;    // (row, col) pairs sorted by (row, col, orientation): all of them, or, with
                                       // count > max_hits, some max_hits of them (truncated)
        std::vector<u8> orientation;   // the id of each pair's template
        bool truncated = false;
    };
    MatchResult match(const std::vector<std::pair<int, MatchTemplate>>& ts, i64 max_hits, bool positions);
    // dst (h x w dense cells, as read_tile_cells takes them): 1 where any template of `ts` matches, else 0.
    void match_cells(const std::vector<std::pair<int, MatchTemplate>>& ts, const CellBuffer& dst);
    // ----- connected components (gol/components.hpp) -----
    // The objects of the current board (a Generations rule: of its live plane), torus or bounded as the engine runs.  One
    // rank only, refused as match() refuses; max_objects < 1 and a board of 2^31 cells or more are refused too, all before
    // anything is launched.  want_records = false returns the count alone.  HIP: the kernels of components_kernel.hip;
    // only the counter and the records leave the device.
    ComponentsResult components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records);
    // dst: h x w labels (i32, or i64 with int64) in row-major order, in the backend's kind of memory as the dense cells
    // are; numel must be h * w.
    void components_labels(CcNeighbourhood nb, void* dst, bool int64, i64 numel);

    // ----- dense cells: the tensor readers and writers (gol/cells.hpp) -----
    // The caller's buffer is one element per cell (u8, f16, bf16 or f32; exact 0 and 1 out, != 0 alive in).  HIP
    // backend: device memory of the engine's device, verified with hipPointerGetAttributes before anything is launched,
    // and the conversion is a kernel (src/hip/tensor_kernels.hip); CPU backend: host memory and a host loop.  Every call
    // checks numel against the cells it moves, enqueues on the engine's compute stream and synchronises it before
    // returning.  The tile and envelope calls act on this rank's own tile on any rank count; the window and film calls
    // are for one rank and throw, naming the rank count, on more (summing the ranks' parts on the device is not built).
    void read_tile_cells(const CellBuffer& dst);      // h x w cells of this rank's tile
    void read_envelope_cells(const CellBuffer& dst);  // this rank's tile of the envelope (envelope mode)
    // set_tile_words() from dense cells, with everything it does afterwards: ghost refresh, envelope reset; the
    // per-generation records run on.
    void write_tile_cells(const CellBuffer& src);
    // window()'s rectangle and checks; the seams are crossed by addressing (the rectangle's at most four pieces in one launch)
    void read_window_cells(i64 r0, i64 c0, i64 rows, i64 cols, const CellBuffer& dst);
    // Film mode: `generations` generations, their frames (generations x rows x cols cells) unpacked on the way into dst
    // instead of recorded: run() in chunks of film_chunk() generations, each chunk's packed frames converted at its
    // frame offset and dropped.  Needs an empty film record (throws, saying to call film_clear() first); ends as
    // film_clear() does, with an empty record that starts at the generation reached.
    void run_film_cells(u64 generations, const CellBuffer& dst);
    CellSource tile_source(const u64* buf, i64 r0, i64 c0, i64 rows, i64 cols) const;  // a rectangle of a buffer in layout L_
    CellSource film_source(const u64* frames, i64 words, i64 n) const;                // n packed frames (gol/film.hpp)

    // Collective: align the ranks right before a timed region.  Host barrier; with a device
    // transport also a 1-element all-reduce on the compute stream, waited for, so every rank leaves
    // when the collective has completed on the GPUs, not when a host barrier happened to release it.
    virtual void device_barrier() { t_->barrier(); }
    // The end of a timed region: every GPU stream of this rank drained (HIP: device-wide when the device
    // is not shared with other ranks of the process, as torch.cuda.synchronize() in bench.py).
    virtual void device_sync() { synchronize(); }
    // Collective: `reps` timed runs of `gens` generations on the live board (it advances), each bracketed
    // as bench.py brackets its timed run (device_barrier, the run, device_sync); us per generation, max
    // over the ranks.  Used by the HIP engine's init-time prediction and by tools/predict_gap.py.
    std::vector<double> time_runs(u64 gens, int reps);
    // Collective, untimed: per-phase GPU costs of a k-generation superstep of the schedule in use, in
    // us: "exchange_us" (the halo exchange alone, when there is one) and "superstep_us" (a whole
    // superstep, exchange included), each the best of a few rounds.  Runs on scratch state: the
    // board and the generation count are unchanged.  Empty on backends without a GPU clock.
    virtual std::map<std::string, double> phase_probe(int k) {
        (void)k;
        return {};
    }

    const Geometry& geometry() const { return g_; }
    const Layout& layout() const { return L_; }
    const EngineConfig& config() const { return cfg_; }
    Transport& transport() { return *t_; }
    std::shared_ptr<Transport> transport_ptr() { return t_; }
    const EngineStats& stats() const { return stats_; }
    u64 generation() const { return gen_; }
    std::string describe() const;
    virtual std::string backend_name() const = 0;

    // One halo region in tile coordinates (rows [r0, r0+rows), words [c0, c0+words); c0 may be -1).
    struct Rect {
        i64 r0, rows, c0, words;
        i64 count() const { return rows * words; }
    };
    struct HaloItem {
        Dir d;
        int send_peer, recv_peer;
        Rect send, recv;
        bool contiguous;  // full-pitch rows: can be sent straight from the board
    };
    // Canonical-order halo messages of a k-deep superstep (self directions omitted).
    std::vector<HaloItem> halo_items(int k) const;
    // Halo layout: 2-D blocks (column halos, 8 directions) or 1-D row strips.
    bool two_d() const { return g_.dec.Px > 1 || (xchg_self_ && g_.dec.want_2d); }
    // Directions whose neighbour is this rank wrap by addressing (no messages), unless the
    // self-exchange mode routes them through the transport (x only has halos in the 2-D layout).
    bool self_x() const {
        return g_.nbr[DIR_W] == g_.rank && g_.nbr[DIR_E] == g_.rank && !(xchg_self_ && two_d());
    }
    bool self_y() const { return g_.nbr[DIR_N] == g_.rank && g_.nbr[DIR_S] == g_.rank && !xchg_self_; }
    // (not on a bounded board: a halo lane that streamed word nw - 1 could not tell that it is outside the board)
    bool xwrap_by_plan() const { return self_x() && L_.aligned() && !dead_edges(); }
    bool dead_edges() const { return cfg_.boundary == Boundary::Dead; }
    // Rows of the smallest tile of the job (identical on every rank).
    i64 min_tile_rows() const {
        i64 m = g_.dec.H;
        for (int i = 0; i < g_.dec.Py; ++i) m = std::min(m, g_.dec.row_starts[i + 1] - g_.dec.row_starts[i]);
        return m;
    }

   protected:
    Engine(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t);
    virtual void do_init(const PatternSpec& p) = 0;
    virtual void do_superstep(int k) = 0;
    // Compat mode: install constant depth-1 ghost rows (both buffers); rows are full-pitch.
    virtual void do_set_compat_halos(const std::vector<u64>& above, const std::vector<u64>& below) = 0;
    virtual std::vector<u64> read_row(i64 r) = 0;  // full-pitch row r of the current buffer
    // Largest superstep depth <= want that the backend can run (HIP: instantiated kernel depths).
    virtual int supported_depth(int want) const { return want; }
    // Generations per full superstep (<= the halo depth R; HIP: a multiple of the tuned pass depth
    // when the rank has no neighbours, so no superstep ends with a short, slow pass).
    virtual int superstep_depth() const { return L_.R; }
    void setup_compat();
    void maybe_inject_fault();
    // Watchdog mode: a superstep (or graph replay) has been issued: record its progress marker
    // (backend hook) and kick the watchdog.  No-op without a watchdog.
    void progress(const char* next_phase);
    virtual void note_progress() {}
    // Watchdog probe, run on the watchdog thread (watchdog.hpp): GPU progress markers retired so far,
    // outstanding GPU work, and the data plane's asynchronous error state.
    virtual Watchdog::Probe probe() {
        Watchdog::Probe p;
        p.error = t_->async_error();
        return p;
    }
    [[noreturn]] void fatal(const std::string& what, int code);
    struct Armed {  // arms the watchdog (if any) for the lifetime of a run() / init() / synchronize() call
        explicit Armed(Watchdog* w) : w_(w) {
            if (w_) w_->arm(true);
        }
        ~Armed() {
            if (w_) w_->arm(false);
        }
        Watchdog* w_;
    };

    // Census record of this rank: the counts already on the host; a backend that keeps counts elsewhere (HIP: a
    // device buffer the kernels add into) appends them in census_collect() and drops them in census_discard().
    // (signature mode: census_host_ holds the populations, sig_host_ the signatures, of the same generations)
    virtual void census_collect() {}
    virtual void census_discard() {}
    std::vector<u64> census_host_, sig_host_;
    std::vector<u64> film_host_;  // film mode: this rank's packed frames, film_geo_.slot_words() words each
    FilmGeo film_geo_;
    std::vector<u64> density_host_;  // density-film mode: this rank's maps, density_geo_.slot_words() words each
    DensityGeo density_geo_;
    u64 census_start_ = 0;
    void sum_series(std::vector<u64>& series, const char* what);  // collective: the ranks' series added up (wrapping)
    // This rank's part of signature(), snapshot() and snapshot_diff().
    virtual u64 local_signature() = 0;
    virtual void snapshot_local() = 0;
    virtual u64 snapshot_diff_local() = 0;
    bool have_snapshot_ = false;
    // Envelope mode.  envelope_merge_local: E = (reset ? 0 : E) | the tile's own cells of the current board.
    // view_env_: tile_words(), read_window_local(), density_local() and local_reduce() read E instead of the board
    // (set for the length of an envelope_* reader).
    virtual void envelope_merge_local(bool reset) = 0;
    void envelope_reset();  // start = generation(), E = the current board
    void need_envelope(const char* what) const;
    bool view_env_ = false;
    u64 env_start_ = 0;
    // Generations rules.  view_plane_: the plane tile_words(), read_window_local(), density_local() and local_reduce()
    // read (0: the live plane; set for the length of a state reader).  write_planes_local: the tile's 1 + M planes from
    // dense natural-order words (h * nw each; a null entry: zeros), then what set_tile_words() does after its copy.
    // settle_decay_local: every decay plane ANDed with the complement of the live plane over the tile, ghosts refreshed.
    // state_counts_local: counts[s] += this rank's cells in state s.
    int view_plane_ = 0;
    virtual void write_planes_local(const std::vector<const u64*>& planes) = 0;
    virtual void settle_decay_local() = 0;
    virtual void state_counts_local(u64* counts) = 0;
    void need_generations(const char* what) const;
    // Dense cells: the backends' parts.  check_cell_pointer: throw unless the buffer's memory is the backend's kind
    // (HIP: device memory of the engine's device; CPU: nothing to ask).  read_rect_cells: the rectangle of the board
    // (view_env_: the envelope) in tile coordinates, wrapping at the tile's edges.  write_tile_cells_local: the cells
    // into the tile, then what set_tile_words() does after its copy.  film_chunk: the generations run_film_cells() runs
    // between two drains; film_drain_cells: the `frames` frames run() has just recorded, converted into dst from frame
    // `at` on, and the record empty again.
    virtual void check_cell_pointer(const CellBuffer& b, const char* what) = 0;
    virtual void read_rect_cells(i64 r0, i64 c0, i64 rows, i64 cols, const CellBuffer& dst) = 0;
    virtual void write_tile_cells_local(const CellBuffer& src) = 0;
    virtual size_t film_chunk() const = 0;
    virtual void film_drain_cells(size_t frames, const CellBuffer& dst, size_t at) = 0;
    // Pattern matching: the backends' parts.  match_local: run the matcher for one template on the current board and
    // return its matches; with keep, the backend's bitmap then holds them (or_into: ORed into what it held).
    // match_positions_local: `cap` (row, col) pairs of the bitmap's set bits (cap <= their number) appended to out.
    // match_bitmap_cells: the bitmap as dense cells.
    virtual u64 match_local(const MatchTemplate& t, bool keep, bool or_into) = 0;
    virtual void match_positions_local(i64 cap, std::vector<i32>* out) = 0;
    virtual void match_bitmap_cells(const CellBuffer& dst) = 0;
    void check_match(const std::vector<std::pair<int, MatchTemplate>>& ts, const char* what) const;
    // Connected components: the backends' parts, on the current board.
    virtual ComponentsResult components_local(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) = 0;
    virtual void components_labels_cells(CcNeighbourhood nb, void* dst, bool int64) = 0;
    void check_components(i64 max_objects, const char* what) const;

    Geometry g_;
    EngineConfig cfg_;
    std::shared_ptr<Transport> t_;
    Layout L_;
    EngineStats stats_;
    u64 gen_ = 0;
    i64 fault_gen_ = -1;
    std::string fault_mode_ = "abort";  // GOL_FAULT=rank:gen[:abort|hang|exit]
    std::unique_ptr<Watchdog> wd_;
    bool xchg_self_ = false;  // cfg_.self_exchange (not in compat mode)
};

std::unique_ptr<Engine> make_cpu_engine(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t);
std::unique_ptr<Engine> make_hip_engine(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t);

// HIP runtime helpers used by the CLI / bindings (no-ops without a GPU).
int hip_device_count(int* err = nullptr);
void hip_set_device(int dev);
int hip_try_set_device(int dev);  // hipError_t of hipSetDevice (0 = success)

}  // namespace gol
