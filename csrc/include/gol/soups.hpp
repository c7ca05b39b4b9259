// gol-mi355x: soup batches -- many small independent square tori per launch, each run until it settles.
//
// A batch is n tori of side S = 64 m (m = 1, 2, 4) under one Moore rule.  It is not an Engine: there is no
// plan, transport, schedule or autotune.  All per-soup state lives in the backend's memory between calls (the
// board, the saved board of the search, the initial board, the search's counters and the result record), so a
// run can be cut into launches of at most `chunk` generations and continued by later calls with the same result.
//
// Settling is Brent's search with exact board comparison (no hash): a soup keeps a copy of its board saved at
// generation s and a window w, at first s = origin, w = 1.  After each step to generation g: board == copy means
// settled with period g - s at generation g; otherwise g - s == w saves the board, s = g, w *= 2.  The saves fall
// at origin + 2^k - 1, and the first hit after a save on the cycle is the least period.  A soup that reaches
// max_gens unsettled has period 0.  The exact transient (optional) restarts two copies of a settled soup from the
// initial board, advances one by the period and steps both until they are equal.
// The origin is generation 0, or the generation step() had reached when settle() was first called: step() is the
// plain stepper (no comparison) and is refused once a search has begun, since settled soups stop at different
// generations.
//
// Backends of identical results: "hip" (step_soups, src/hip/soup_kernel.hip: one wave64 per soup, the board in
// registers, no memory traffic, LDS or barrier inside a launch) and "cpu" (src/cpu/soups_cpu.cpp: the same
// per-soup program on packed words, OpenMP over the soups).
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "gol/cells.hpp"
#include "gol/common.hpp"
#include "gol/components.hpp"
#include "gol/match.hpp"
#include "gol/rule.hpp"

namespace gol {

constexpr i64 kSoupsMax = (i64)1 << 20;           // soups per batch
constexpr u64 kSoupMaxGens = (u64)1 << 31;        // the search's counters are 32-bit
constexpr i64 kSoupDefaultChunk = 4096;           // generations per launch

// One soup's state, as the backends keep it (32 bytes; the HIP kernel reads and writes it as it stands).
struct alignas(16) SoupState {
    u32 g = 0;           // generation of the board
    u32 s = 0;           // generation of the saved copy
    u32 w = 1;           // window: the copy is replaced when g - s == w
    u32 period = 0;      // 0: not settled (yet)
    u32 population = 0;  // live cells of the board at generation g
    u32 flags = 0;       // kSoupTransient*
    u32 tadv = 0;        // transient phase: generations the second copy is ahead (up to period)
    u32 tcount = 0;      // transient phase: steps both copies have taken
};
enum : u32 { kSoupTransientStarted = 1u << 0, kSoupTransientDone = 1u << 1 };

struct SoupRecord {
    u32 period;      // 0: not settled by `generation`
    i64 transient;   // -1: not computed (no transient=true, or not settled)
    u32 generation;  // where the soup stopped: the generation of the hit, or max_gens
    u32 population;  // live cells at `generation`
};

struct SoupConfig {
    i64 n = 1;
    i64 size = 64;
    Rule rule;
    std::string boundary = "torus";  // anything else is refused
    bool compat = false;             // refused
    std::string backend = "hip";     // hip | cpu
    int device = 0;
    int workgroup = 0;               // HIP: threads per workgroup, 64 | 128 | 256 (0: GOL_SOUPS_WG, else 64)
};

struct SoupStats {
    std::string kernel;   // soups@64, soups@128, soups@256; ":rule" appended for the generic variant
    std::string backend;
    std::string rule;
    u64 launches = 0;     // kernel launches (CPU: parallel sweeps) of step() and settle()
    u64 settled = 0;      // soups settled so far
    u64 reached = 0;      // generation of the soups not settled
    int workgroup = 0;
};

class SoupBatch {
   public:
    // Validates the configuration (throws gol::Error naming the offending value) before anything is allocated.
    static std::unique_ptr<SoupBatch> create(const SoupConfig& c);
    static void validate(const SoupConfig& c);
    virtual ~SoupBatch() = default;

    i64 n() const { return cfg_.n; }
    i64 size() const { return cfg_.size; }
    int m() const { return (int)(cfg_.size / 64); }
    i64 words_per_soup() const { return cfg_.size * m(); }
    const SoupConfig& config() const { return cfg_; }

    // Soup i starts as pattern 5 (random_word, common.hpp) of seed + i (mod 2^64).
    void init_seed(u64 seed);
    // n * S * m natural-order words (bit b of word c of a row = column 64 c + b), soup after soup, row after row.
    void init_words(const u64* natural);

    // g generations of every soup, no comparison.  Refused after settle() has begun a search.
    void step(u64 g);
    // Runs every unsettled soup until it settles or stands at generation max_gens, at most `chunk` generations per
    // launch; with `transient`, then finds the exact transient of every settled soup that has none yet.
    void settle(u64 max_gens, bool transient = false, i64 chunk = kSoupDefaultChunk);

    std::vector<SoupRecord> records();
    // The boards of the soups idx (0 <= idx < n), one byte per cell, (k, S, S).
    std::vector<u8> boards(const std::vector<i64>& idx);
    // Dense cells (gol/cells.hpp; HIP: device memory of the batch's device, verified before anything is launched, and a
    // kernel of src/hip/tensor_kernels.hip; CPU: host memory, a host loop).  Both check numel, run on the batch's stream
    // and synchronise it before returning.
    // The boards of the soups first .. first + count - 1 as (count, S, S) elements, exact 0 and 1.
    void read_boards_cells(i64 first, i64 count, const CellBuffer& dst);
    // init_words() from (n, S, S) elements, alive iff != 0.
    void init_cells(const CellBuffer& src);
    // Pattern matching (gol/match.hpp): n x T counts, entry (i, t) the matches of the oriented templates templates[t],
    // summed, on soup i's current board (a torus).  Every template is validated against the soup's size before anything
    // runs.  HIP: the batch's stream is synchronised first (a pending step() is included), then one k_match launch per
    // oriented template over all soups adds into one counter per soup; no bitmap is kept.
    std::vector<u32> match_counts(const std::vector<std::vector<MatchTemplate>>& templates);
    // Connected components (gol/components.hpp) of every soup's current board, each its own torus: the records carry the
    // soup's index, anchors and boxes are in the soup's own coordinates, per_board holds the objects of every soup.
    // max_objects < 1 and n * S * S >= 2^31 are refused before anything runs.  HIP: the batch's stream is synchronised
    // first (a pending step() is included), then the kernels of components_kernel.hip run over the whole store.
    ComponentsResult components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records);
    SoupStats stats() const;
    // Waits for the launches of step() (HIP; every other call returns finished work).
    virtual void synchronize() {}

   protected:
    explicit SoupBatch(const SoupConfig& c) : cfg_(c) {}

    // Backend hooks.  Boards travel in split storage (bits.hpp), soup after soup, row after row.
    virtual void do_init_seed(u64 seed) = 0;
    virtual void do_upload(const u64* split) = 0;
    virtual void do_plain(u32 gens) = 0;                      // every soup: gens steps, population
    virtual void do_begin_search() = 0;                       // initial = saved = board; s = g, w = 1
    virtual u64 do_settle(u32 gens, u32 max_gens) = 0;        // one launch; returns the soups settled so far
    virtual u64 do_transient(u32 gens) = 0;                   // one launch; returns the settled soups still without
    virtual void do_fetch_states(SoupState* out) = 0;
    virtual void do_fetch_board(i64 soup, u64* split) = 0;
    virtual void do_read_cells(i64 first, i64 count, const CellBuffer& dst) = 0;
    virtual void do_init_cells(const CellBuffer& src) = 0;  // the boards and, as do_upload, the states
    // counts[i] = the matches of the templates, summed, on soup i's board (n counts)
    virtual void do_match_counts(const std::vector<MatchTemplate>& oriented, u32* counts) = 0;
    virtual ComponentsResult do_components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) = 0;
    // the soups first .. first + count - 1 of a store of n x S x m words
    CellSource soup_source(const u64* store, i64 first, i64 count) const;
    CellTarget soup_target(u64* store) const;

    SoupConfig cfg_;
    bool searching_ = false;
    u64 reached_ = 0;  // generation of every soup that is not settled
    u64 launches_ = 0, settled_ = 0;
};

// The backends' factories (create() dispatches; the HIP one throws when there is no device).
std::unique_ptr<SoupBatch> make_cpu_soups(const SoupConfig& c);
std::unique_ptr<SoupBatch> make_hip_soups(const SoupConfig& c);

}  // namespace gol
