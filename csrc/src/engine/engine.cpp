// gol-mi355x: engine base (superstep loop, halo plan, compat mode, fault injection) + CPU backend.
#include "gol/engine.hpp"

#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "gol/bits.hpp"
#include "gol/cpu.hpp"
#include "gol/trace.hpp"

namespace gol {

// ---------------------------------------------------------------------------------------------
// Base
// ---------------------------------------------------------------------------------------------

Engine::Engine(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t)
    : g_(g), cfg_(c), t_(std::move(t)) {
    if (!t_) throw Error("engine needs a transport");
    xchg_self_ = cfg_.self_exchange && !cfg_.compat;
    Rule::from_masks(cfg_.rule.birth, cfg_.rule.survive, cfg_.rule.nbhd, cfg_.rule.states);  // (a rule set by its masks: range and B0 checks)
    if (cfg_.rule.generations()) {
        // A Generations rule is a mode of its own: one rank, no in-kernel record, the generic streaming pass only.
        const std::string rs = cfg_.rule.str();
        auto refuse = [&rs](const char* option, const char* why) {
            throw Error(std::string(option) + " with the Generations rule " + rs + ": " + why);
        };
        if (g_.dec.P > 1)
            throw Error(strprintf("the Generations rule %s on %d ranks: Generations rules run on one rank (the exchange of the "
                                  "decay planes is not built)", rs.c_str(), g_.dec.P));
        if (cfg_.census) refuse("census", "the census kernel counts two-state boards");
        if (cfg_.signature) refuse("signature", "the signature kernel hashes two-state boards");
        if (cfg_.film.on) refuse("film", "the film kernel stores two-state frames");
        if (cfg_.density_film.on) refuse("density_film", "the density kernel counts two-state boards");
        if (cfg_.envelope) refuse("envelope", "the envelope kernel records two-state boards");
        if (cfg_.compat) refuse("compat (GOL_COMPAT=reference)", "the reference has one rule, B3/S23");
        if (cfg_.subtiles == 2) refuse("subtiles=2 (GOL_SUBTILES=2)", "the sub-tile halves run B3/S23 only");
        if (cfg_.self_exchange) refuse("self_exchange (GOL_SELF_EXCHANGE)", "the exchange of the decay planes is not built");
        if (cfg_.force_split) refuse("force_split (GOL_FORCE_SPLIT)", "the split schedule's exchange of the decay planes is not built");
        if (cfg_.backend == "hip" && cfg_.kernel != "auto" && cfg_.kernel != "rule")
            refuse(("kernel '" + cfg_.kernel + "'").c_str(), "step_gen runs every pass (use kernel auto or rule)");
    }
    if (cfg_.rule.ltl()) {
        // A Larger than Life rule is a mode of its own too: one rank, one generation per superstep and per pass, no
        // in-kernel record.  (Checkpoints and the rank agreement need Rule::code(), which such a rule does not have.)
        const Rule& r = cfg_.rule;
        Rule::from_ltl(r.range, r.middle, r.smin, r.smax, r.bmin, r.bmax);  // (a rule set by its fields: parse's checks)
        const std::string rs = r.str();
        auto refuse = [&rs](const std::string& option, const char* why) {
            throw Error(option + " with the Larger than Life rule " + rs + ": " + why);
        };
        if (g_.dec.P > 1)
            throw Error(strprintf("the Larger than Life rule %s on %d ranks: Larger than Life rules run on one rank (the exchange of "
                                  "halos of depth R is not built)", rs.c_str(), g_.dec.P));
        if (cfg_.census) refuse("census", "the census kernel counts inside the radius-1 kernels");
        if (cfg_.signature) refuse("signature", "the signature kernel hashes inside the radius-1 kernels");
        if (cfg_.film.on) refuse("film", "the film kernel stores frames inside the radius-1 kernels");
        if (cfg_.density_film.on) refuse("density_film", "the density kernel counts inside the radius-1 kernels");
        if (cfg_.envelope) refuse("envelope", "the envelope kernel records inside the radius-1 kernels");
        if (cfg_.compat) refuse("compat (GOL_COMPAT=reference)", "the reference has one rule, B3/S23");
        if (cfg_.subtiles == 2) refuse("subtiles=2 (GOL_SUBTILES=2)", "the sub-tile halves run B3/S23 only");
        if (cfg_.self_exchange) refuse("self_exchange (GOL_SELF_EXCHANGE)", "the exchange of halos of depth R is not built");
        if (cfg_.force_split) refuse("force_split (GOL_FORCE_SPLIT)", "the split schedule is not built for a box of range R");
        if (cfg_.backend == "hip" && cfg_.kernel != "auto" && cfg_.kernel != "rule")
            refuse("kernel '" + cfg_.kernel + "'", "step_ltl runs every pass (use kernel auto or rule)");
        if (cfg_.kernel_depth != 0 && cfg_.kernel_depth != 1)
            refuse(strprintf("kernel_depth %d (GOL_KERNEL_DEPTH)", cfg_.kernel_depth), "a pass is one generation (auto or 1)");
        if (cfg_.halo_depth > 1)
            refuse(strprintf("halo_depth %d (GOL_HALO_DEPTH)", cfg_.halo_depth), "a superstep is one generation (auto or 1)");
        const i64 side = 2 * (i64)r.range + 1;
        if (g_.dec.H < side || g_.dec.W < side)
            throw Error(strprintf("rule %s on a %lld x %lld board: the box of range %d needs a board of at least %lld x %lld cells, "
                                  "so that no neighbour is counted twice", rs.c_str(), (long long)g_.dec.H, (long long)g_.dec.W,
                                  (int)r.range, (long long)side, (long long)side));
    }
    if (!cfg_.rule.is_conway() && !cfg_.rule.ltl()) {
        const std::string rs = cfg_.rule.str();
        if (cfg_.compat) throw Error("GOL_COMPAT=reference with rule " + rs + ": the reference has one rule, B3/S23");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) run B3/S23 only, not rule " + rs);
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' implements B3/S23 only, not rule " + rs +
                                " (use kernel auto or rule)");
    }
    if (cfg_.boundary != Boundary::Torus && cfg_.boundary != Boundary::Dead)
        throw Error(strprintf("boundary must be torus or dead (got the value %d)", (int)cfg_.boundary));
    if (dead_edges()) {
        if (cfg_.compat) throw Error("GOL_COMPAT=reference with boundary dead: the reference is a torus");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) implement the torus only, not boundary dead");
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' implements the torus only, not boundary dead (use kernel auto or rule)");
    }
    if (cfg_.census) {
        if (cfg_.compat) throw Error("census with GOL_COMPAT=reference: compat mode runs the reference's loop, not the census kernel");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) do not run the census kernel");
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' counts no census: the census kernel runs every pass (use kernel auto or rule)");
    }
    if (cfg_.signature) {
        if (cfg_.census) throw Error("signature together with census: signature mode already records the population of every generation");
        if (cfg_.compat) throw Error("signature with GOL_COMPAT=reference: compat mode runs the reference's loop, not the signature kernel");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) do not run the signature kernel");
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' records no signatures: the signature kernel runs every pass (use kernel auto or rule)");
    }
    if (cfg_.film.on) {
        const FilmRect& f = cfg_.film;
        if (cfg_.census) throw Error("film together with census: one per-generation record per engine (film mode stores frames, not counts)");
        if (cfg_.signature) throw Error("film together with signature: one per-generation record per engine (film mode stores frames, not hashes)");
        if (cfg_.compat) throw Error("film with GOL_COMPAT=reference: compat mode runs the reference's loop, not the film kernel");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) do not run the film kernel");
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' stores no frames: the film kernel runs every pass (use kernel auto or rule)");
        check_window(f.r0, f.c0, f.rows, f.cols);  // (window()'s checks: names the rectangle and the board)
        if (f.rows * f.cols > kFilmMaxCells)
            throw Error(strprintf("film: a window of %lld x %lld cells has more than 2^22 cells; read larger rectangles with window()",
                                  (long long)f.rows, (long long)f.cols));
        film_geo_ = FilmGeo(f, g_.dec.H, g_.dec.W);
    }
    if (cfg_.density_film.on) {
        const DensityBlocks& b = cfg_.density_film;
        if (cfg_.census) throw Error("density_film together with census: one per-generation record per engine (density-film mode stores maps, not one count)");
        if (cfg_.signature) throw Error("density_film together with signature: one per-generation record per engine (density-film mode stores maps, not hashes)");
        if (cfg_.film.on) throw Error("density_film together with film: one per-generation record per engine (density-film mode stores maps, not frames)");
        if (cfg_.compat) throw Error("density_film with GOL_COMPAT=reference: compat mode runs the reference's loop, not the density kernel");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) do not run the density kernel");
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' counts no density maps: the density kernel runs every pass (use kernel auto or rule)");
        // density()'s checks; the one of a block's size first, in words that name the shape
        if (b.rows >= 1 && b.cols >= 64 && b.cols % 64 == 0 &&
            std::min(b.rows, g_.dec.H) > (i64)0xFFFFFFFFll / std::min(b.cols, round_up(g_.dec.W, 64)))
            throw Error(strprintf("density_film: a block of %lld x %lld cells on the %lld x %lld board holds more than 2^32 - 1 cells, "
                                  "its count would not fit",
                                  (long long)b.rows, (long long)b.cols, (long long)g_.dec.H, (long long)g_.dec.W));
        check_density(b.rows, b.cols);
        if (ceil_div(g_.dec.H, b.rows) > kDensityFilmMaxBlocks / ceil_div(g_.dec.W, b.cols))
            throw Error(strprintf("density_film: blocks of %lld x %lld cells make a grid of %lld x %lld blocks, more than 2^20 per "
                                  "generation; read finer grids with density()",
                                  (long long)b.rows, (long long)b.cols, (long long)ceil_div(g_.dec.H, b.rows),
                                  (long long)ceil_div(g_.dec.W, b.cols)));
        density_geo_ = DensityGeo(b, g_.dec.H, g_.dec.W);
    }
    if (cfg_.envelope) {
        if (cfg_.census) throw Error("envelope together with census: one in-kernel record per engine (envelope mode keeps one OR, not counts)");
        if (cfg_.signature) throw Error("envelope together with signature: one in-kernel record per engine (envelope mode keeps one OR, not hashes)");
        if (cfg_.film.on) throw Error("envelope together with film: one in-kernel record per engine (envelope mode keeps one OR, not frames)");
        if (cfg_.density_film.on) throw Error("envelope together with density_film: one in-kernel record per engine (envelope mode keeps one OR, not maps)");
        if (cfg_.compat) throw Error("envelope with GOL_COMPAT=reference: compat mode runs the reference's loop, not the envelope kernel");
        if (cfg_.subtiles == 2) throw Error("two sub-tiles per rank (GOL_SUBTILES=2) do not run the envelope kernel");
        if (cfg_.backend == "hip")
            for (const char* k : {"temporal", "tile", "pipe", "resident", "lds"})
                if (cfg_.kernel == k)
                    throw Error("kernel '" + cfg_.kernel + "' keeps no envelope: the envelope kernel runs every pass (use kernel auto or rule)");
    }
    if (t_->size() != g_.dec.P || t_->rank() != g_.rank)
        throw Error(strprintf("transport (rank %d of %d) does not match the geometry (rank %d of %d)", t_->rank(),
                              t_->size(), g_.rank, g_.dec.P));
    // auto depth: 32 generations per superstep (the tile-kernel autotune tries passes of up to 32
    // on one rank); with neighbours (or self-exchange, which stands in for them on one GPU), 128 for
    // 1-D strips of >= 2048 rows and 56 for 2-D tiles of >= 2048 rows (the column halo is one word:
    // <= 63): an exchange costs an RCCL kernel plus ~15 us of cross-stream event latency however
    // small it is (kernel traces of the 4096 x 32768 strip of config 3 strong-scaled over 8 GPUs:
    // 11-13 us RCCL + 14 us event wait per superstep, profiles/), while the ghost rows a deeper
    // superstep recomputes cost < 1.5% at 2048 rows.
    // The HIP backend runs a superstep as kernel passes of K (auto 8) generations (deep halos).
    // (from the average strip height, identical on every rank: all ranks must cut the same
    // supersteps, and uneven strips differ by a row)
    const i64 strip_rows = g_.dec.H / std::max(1, g_.dec.Py);
    const bool nbrs = g_.dec.P > 1 || xchg_self_;
    const bool tall_strips = nbrs && !two_d() && strip_rows >= 2048;
    const bool tall_tiles = nbrs && two_d() && strip_rows >= 2048;
    // ... and 128 when the two-sub-tile mode can run (HIP, GOL_SUBTILES auto or 2, 1-D tiles of >=
    // 24576 rows, aligned width, no measurement / compat mode; any transport: device transports
    // run the halves' exchange stream ordered, host transports stage it): its halves wait for each
    // other once per superstep (a kernel trace
    // showed ~47 us of one queue and ~12 us of both idle at every boundary), so longer supersteps
    // pay that less often: 32768^2, 2048 generations, 10.01-10.05 us/gen at 64, 9.94-9.98 at 96,
    // 9.70-9.79 at 128 (profiles/subtile_superstep_boundaries.txt).  Rank-invariant inputs only.
    const bool sub_tall = cfg_.backend == "hip" && (cfg_.subtiles == 2 || cfg_.subtiles < 0) && !two_d() && strip_rows >= kSubtileMinRows &&
                          g_.dec.W % 64 == 0 && !cfg_.force_split && !cfg_.profile && !cfg_.compat &&
                          cfg_.kernel != "lds" && cfg_.kernel != "tile" && cfg_.kernel != "pipe" &&
                          cfg_.kernel != "rule" && cfg_.rule.is_conway() && !dead_edges() && !recording();
    // (1-D strips with neighbours: 128 measured 1-3% faster than 64 through RCCL self-exchange,
    // 4096 x 32768 2.44 -> 2.36, 8192 x 65536 5.93 -> 5.85 us/gen; profiles/per_rank_tiles_self_exchange.txt)
    const int want = cfg_.halo_depth > 0 ? cfg_.halo_depth : (sub_tall || tall_strips ? 128 : (tall_tiles ? 56 : 32));
    int R = clamp_halo_depth(g_.dec, want);
    // A Larger than Life generation of range r has the dependency cone of r Life generations: the layout's halo depth is
    // r, so that slack rows and ghost words exist as for a pass of depth r; the superstep itself is one generation.
    if (ltl()) R = clamp_halo_depth(g_.dec, (int)cfg_.rule.range);
    if (two_d()) R = std::min(R, 63);  // the column halo is one 64-cell word
    if (cfg_.compat) {
        if (two_d()) throw Error("GOL_COMPAT=reference supports 1-D row strips only");
        R = 1;
    }
    L_ = Layout(g_.h, g_.w, R);
    stats_.depth = ltl() ? 1 : R;
    stats_.rule = cfg_.rule.str();
    stats_.states = (int)cfg_.rule.states;
    stats_.boundary = boundary_name(cfg_.boundary);
    stats_.census = cfg_.census;
    stats_.signature = cfg_.signature;
    stats_.film = cfg_.film;
    stats_.density_film = cfg_.density_film;
    stats_.envelope = cfg_.envelope;
    std::string f = env_str("GOL_FAULT", "");
    if (!f.empty()) {
        int fr = -1;
        long long fg = -1;
        char mode[16] = {0};
        const int n = sscanf(f.c_str(), "%d:%lld:%15s", &fr, &fg, mode);
        if (n >= 2 && fr == g_.rank) {
            fault_gen_ = fg;
            if (n == 3) fault_mode_ = mode;
            if (fault_mode_ != "abort" && fault_mode_ != "hang" && fault_mode_ != "exit")
                throw Error("GOL_FAULT mode must be abort, hang or exit (got '" + fault_mode_ + "')");
        }
    }
    if (cfg_.watchdog_s > 0) {
        // (the probe is a virtual call on the watchdog thread: it is enabled at the end of init(),
        // once the backend is fully constructed, and backends stop the watchdog first on destruction)
        wd_ = std::make_unique<Watchdog>(
            cfg_.watchdog_s, [this](const std::string& what) { fatal("watchdog: " + what, 4); },
            [this] { return probe(); });
    }
}

void Engine::fatal(const std::string& what, int code) {
    fprintf(stderr, "[gol] rank %d, generation %llu: %s; aborting the job\n", g_.rank, (unsigned long long)gen_,
            what.c_str());
    fflush(stderr);
    // The transport's abort (ncclCommAbort, MPI_Abort, socket teardown) must not be able to hang
    // the exit: a last-resort timer ends the process regardless.
    std::thread([code] {
        std::this_thread::sleep_for(std::chrono::seconds(15));
        fprintf(stderr, "[gol] transport abort did not return within 15 s; exiting\n");
        fflush(stderr);
        _exit(code);
    }).detach();
    t_->abort(code);
    _exit(code);  // not reached: Transport::abort does not return
}

void Engine::progress(const char* next_phase) {
    if (!wd_) return;
    note_progress();
    wd_->kick(next_phase);
}

std::unique_ptr<Engine> Engine::create(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t) {
    if (c.backend == "cpu") return make_cpu_engine(g, c, std::move(t));
    if (c.backend == "hip") return make_hip_engine(g, c, std::move(t));
    throw Error("unknown backend '" + c.backend + "' (expected cpu or hip)");
}

std::string Engine::describe() const {
    const std::string wg = cfg_.backend == "hip" ? strprintf(", tile workgroup %d waves", cfg_.tile_waves) : "";
    return strprintf("%s backend, %s, rank %d tile %lldx%lld at (%lld,%lld), halo depth %d, transport %s%s%s, rule %s%s",
                     backend_name().c_str(), g_.dec.describe().c_str(), g_.rank, (long long)g_.h, (long long)g_.w,
                     (long long)g_.row0, (long long)g_.col0, L_.R, t_->name().c_str(), wg.c_str(),
                     cfg_.compat ? ", compat=reference" : "", cfg_.rule.str().c_str(),
                     dead_edges() ? ", boundary dead" : "");
}

std::vector<Engine::HaloItem> Engine::halo_items(int k) const {
    std::vector<HaloItem> items;
    const i64 h = L_.h, nw = L_.nw, P = L_.pitch;
    auto add = [&](Dir d, Rect s, Rect r, bool contig) {
        const int sp = g_.nbr[d], rp = g_.nbr[opposite(d)];
        if (sp == g_.rank && rp == g_.rank && !xchg_self_) return;  // self direction: wrap by addressing
        items.push_back({d, sp, rp, s, r, contig});
    };
    if (!two_d()) {
        if (!self_y()) {
            add(DIR_N, {0, k, -1, P}, {h, k, -1, P}, true);
            add(DIR_S, {h - k, k, -1, P}, {-k, k, -1, P}, true);
        }
    } else {
        if (!self_y()) {
            add(DIR_N, {0, k, 0, nw}, {h, k, 0, nw}, false);
            add(DIR_S, {h - k, k, 0, nw}, {-k, k, 0, nw}, false);
        }
        add(DIR_W, {0, h, 0, 1}, {0, h, nw, 1}, false);
        add(DIR_E, {0, h, nw - 1, 1}, {0, h, -1, 1}, false);
        if (!self_y()) {
            add(DIR_NW, {0, k, 0, 1}, {h, k, nw, 1}, false);
            add(DIR_NE, {0, k, nw - 1, 1}, {h, k, -1, 1}, false);
            add(DIR_SW, {h - k, k, 0, 1}, {-k, k, nw, 1}, false);
            add(DIR_SE, {h - k, k, nw - 1, 1}, {-k, k, -1, 1}, false);
        }
    }
    return items;
}

void Engine::init(const PatternSpec& p) {
    trace::Range range("gol.init");
    Armed armed(wd_.get());
    gen_ = 0;
    stats_ = EngineStats{};
    stats_.depth = ltl() ? 1 : L_.R;
    stats_.kernel = backend_name() == "cpu" ? "cpu" : cfg_.kernel;
    stats_.schedule = halo_items(L_.R).empty() ? "local" : "full";
    stats_.kernel_depth = ltl() ? 1 : L_.R;
    stats_.rule = cfg_.rule.str();
    stats_.states = (int)cfg_.rule.states;
    stats_.boundary = boundary_name(cfg_.boundary);
    stats_.census = cfg_.census;
    stats_.signature = cfg_.signature;
    stats_.film = cfg_.film;
    stats_.density_film = cfg_.density_film;
    stats_.envelope = cfg_.envelope;
    census_restart(0);
    have_snapshot_ = false;
    if (t_->size() > 1) {
        // every rank must run the same rule on the same boundary, in the same census mode: agreed like the schedule,
        // by reductions every rank sees (so on a mismatch every rank raises and none waits for a peer).  One code:
        // the rule's 32 bits, the boundary above them, the census mode above that (exact in a double).
        // (signature mode one bit above the census mode's)
        // (film mode one bit above the signature mode's; the window's four numbers are agreed after the modes)
        const double code = (double)cfg_.rule.code() + (double)((u64)cfg_.boundary << 32) + (double)((u64)cfg_.census << 40) +
                            (double)((u64)cfg_.signature << 41) + (double)((u64)cfg_.film.on << 42) +
                            (double)((u64)cfg_.density_film.on << 43) +  // (density-film mode one bit above the film mode's)
                            (double)((u64)cfg_.envelope << 44);          // (envelope mode one bit above that)
        const double lo = t_->allreduce_min(code), hi = t_->allreduce_max(code);
        if (lo != hi) {
            u64 clo = (u64)lo, chi = (u64)hi;
            if ((clo >> 44) != (chi >> 44))
                throw Error(strprintf("the ranks disagree on the envelope mode: rank %d has envelope %s (some ranks on, some off)",
                                      g_.rank, cfg_.envelope ? "on" : "off"));
            clo &= ((u64)1 << 44) - 1;
            chi &= ((u64)1 << 44) - 1;
            if ((clo >> 43) != (chi >> 43))
                throw Error(strprintf("the ranks disagree on the density-film mode: rank %d has density_film %s (some ranks on, some off)",
                                      g_.rank, cfg_.density_film.on ? "on" : "off"));
            clo &= ((u64)1 << 43) - 1;
            chi &= ((u64)1 << 43) - 1;
            if ((clo >> 42) != (chi >> 42))
                throw Error(strprintf("the ranks disagree on the film mode: rank %d has film %s (some ranks on, some off)", g_.rank,
                                      cfg_.film.on ? "on" : "off"));
            clo &= ((u64)1 << 42) - 1;
            chi &= ((u64)1 << 42) - 1;
            if ((clo >> 41) != (chi >> 41))
                throw Error(strprintf("the ranks disagree on the signature mode: rank %d has signature %s (some ranks on, some off)",
                                      g_.rank, cfg_.signature ? "on" : "off"));
            if ((clo >> 40) != (chi >> 40))
                throw Error(strprintf("the ranks disagree on the census mode: rank %d has census %s (some ranks on, some off)",
                                      g_.rank, cfg_.census ? "on" : "off"));
            const u64 ulo = clo & 0xFFFFFFFFFFull, uhi = chi & 0xFFFFFFFFFFull;
            if ((ulo >> 32) != (uhi >> 32))
                throw Error(strprintf("the ranks disagree on the boundary: rank %d has %s (%s .. %s over the ranks)", g_.rank,
                                      stats_.boundary.c_str(), boundary_name((Boundary)(ulo >> 32)),
                                      boundary_name((Boundary)(uhi >> 32))));
            throw Error(strprintf("the ranks disagree on the rule: rank %d has %s (rule codes 0x%x .. 0x%x over the ranks)",
                                  g_.rank, stats_.rule.c_str(), (unsigned)(ulo & 0xFFFFFFFFu), (unsigned)(uhi & 0xFFFFFFFFu)));
        }
        if (cfg_.film.on) {  // (on every rank or on none: agreed above)
            const i64 mine[4] = {cfg_.film.r0, cfg_.film.c0, cfg_.film.rows, cfg_.film.cols};
            bool same = true;
            for (i64 v : mine) {
                const double vlo = t_->allreduce_min((double)v), vhi = t_->allreduce_max((double)v);
                same = same && vlo == vhi;
            }
            if (!same)
                throw Error(strprintf("the ranks disagree on the film window: rank %d has %lld x %lld cells at (%lld, %lld)", g_.rank,
                                      (long long)mine[2], (long long)mine[3], (long long)mine[0], (long long)mine[1]));
        }
        if (cfg_.density_film.on) {  // (likewise)
            const i64 mine[2] = {cfg_.density_film.rows, cfg_.density_film.cols};
            bool same = true;
            for (i64 v : mine) {
                const double vlo = t_->allreduce_min((double)v), vhi = t_->allreduce_max((double)v);
                same = same && vlo == vhi;
            }
            if (!same)
                throw Error(strprintf("the ranks disagree on the density-film blocks: rank %d has blocks of %lld x %lld cells", g_.rank,
                                      (long long)mine[0], (long long)mine[1]));
        }
    }
    do_init(p);
    if (cfg_.envelope) envelope_reset();  // (after the backend's init-time timing, which leaves the envelope alone)
    if (cfg_.compat) setup_compat();
    if (wd_) wd_->enable_probe();
}

void Engine::setup_compat() {
    // Reference halo semantics (survey Q1-Q3): the rows a rank sends are its GENERATION-0 first/last
    // rows (gol-with-cuda.cu:35-47, never refreshed), posted as Irecv(prev), Irecv(next),
    // Isend(first -> prev), Isend(last -> next) with one tag (gol-main.c:97-107).  Per-pair FIFO
    // matching of that exact order gives, for P >= 3, above = prev.last / below = next.first, and
    // for P <= 2 (prev == next) the swapped above = prev.first / below = next.last.  The ghost
    // rows are therefore constant and are installed once, in both buffers.
    const int prev = g_.nbr[DIR_N], next = g_.nbr[DIR_S];
    std::vector<u64> first = read_row(0), last = read_row(L_.h - 1);
    std::vector<u64> above(first.size()), below(first.size());
    if (t_->size() == 1) {
        above = first;  // FIFO of the two self-sends: first row arrives first
        below = last;
    } else {
        std::vector<Message> sends = {{prev, first.data(), first.size() * 8}, {next, last.data(), last.size() * 8}};
        std::vector<Message> recvs = {{prev, above.data(), above.size() * 8}, {next, below.data(), below.size() * 8}};
        t_->exchange_host(sends, recvs);
    }
    do_set_compat_halos(above, below);
}

void Engine::maybe_inject_fault() {
    if (fault_gen_ >= 0 && (i64)gen_ >= fault_gen_) {
        fprintf(stderr, "[gol] GOL_FAULT: injected %s on rank %d at generation %llu\n", fault_mode_.c_str(), g_.rank,
                (unsigned long long)gen_);
        fflush(stderr);
        if (fault_mode_ == "hang") {
            fault_gen_ = -1;
            for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));  // only a watchdog ends this
        }
        if (fault_mode_ == "exit") _exit(3);  // crash without telling the peers
        t_->abort(3);
    }
}

void Engine::run(u64 generations) {
    trace::Range range("gol.eager");  // (the HIP engine's run() opens "gol.run" before its graph replays)
    Armed armed(wd_.get());
    while (generations > 0) {
        maybe_inject_fault();
        int k = cfg_.compat || ltl() ? 1 : supported_depth((int)std::min<u64>((u64)superstep_depth(), generations));
        {
            trace::Range r("gol.superstep");
            do_superstep(k);
        }
        gen_ += (u64)k;
        generations -= (u64)k;
        stats_.generations += (u64)k;
        stats_.supersteps += 1;
        progress("superstep");
    }
    maybe_inject_fault();
}

std::vector<double> Engine::time_runs(u64 gens, int reps) {
    std::vector<double> v;
    for (int r = 0; r < reps; ++r) {
        device_barrier();
        const auto t0 = std::chrono::steady_clock::now();
        run(gens);
        device_sync();
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        v.push_back(t_->allreduce_max(dt) * 1e6 / (double)std::max<u64>(1, gens));
    }
    return v;
}

u64 Engine::population() { return t_->allreduce_sum(local_reduce().first); }
u64 Engine::fingerprint() { return t_->allreduce_sum(local_reduce().second); }

// ---------------------------------------------------------------------------------------------
// Census (the backends fill census_host_ with this rank's counts; the sum over the ranks is made here)
// ---------------------------------------------------------------------------------------------

std::pair<u64, std::vector<u64>> Engine::census() {
    if (!cfg_.census)
        throw Error("census(): this engine is not in census mode (EngineConfig::census, Simulation(census=True), GOL_CENSUS=1)");
    census_collect();
    std::vector<u64> out = census_host_;
    if (t_->size() == 1) return {census_start_, out};
    // (every rank ran the same generations: the series have one length, checked on rank 0, which tells the others)
    const size_t n = out.size();
    std::vector<std::vector<u8>> all;
    t_->gatherv(out.data(), n * sizeof(u64), &all, 0);
    u64 ok = 1;
    if (g_.rank == 0)
        for (int q = 1; q < t_->size(); ++q) {
            if (all[(size_t)q].size() != n * sizeof(u64)) {
                ok = 0;
                break;
            }
            u64 part = 0;
            for (size_t i = 0; i < n; ++i) {
                memcpy(&part, all[(size_t)q].data() + i * sizeof(u64), sizeof(u64));
                out[i] += part;
            }
        }
    t_->broadcast(&ok, sizeof(ok), 0);
    if (!ok) throw Error("census: the ranks' series differ in length (every rank must run the same generations)");
    if (n > 0) t_->broadcast(out.data(), n * sizeof(u64), 0);
    return {census_start_, out};
}

void Engine::census_clear() {
    if (!cfg_.census) throw Error("census_clear(): this engine is not in census mode");
    census_collect();
    census_restart(census_start_ + (u64)census_host_.size());
}

void Engine::census_restart(u64 generation) {
    census_discard();
    census_host_.clear();
    sig_host_.clear();
    film_host_.clear();
    density_host_.clear();
    census_start_ = generation;
}

// ---------------------------------------------------------------------------------------------
// Film (film mode's record: film_host_, this rank's packed frames; gol/film.hpp)
// ---------------------------------------------------------------------------------------------

Engine::Film Engine::film() {
    if (!cfg_.film.on)
        throw Error("film(): this engine is not in film mode (EngineConfig::film, Simulation(film=(r0, c0, rows, cols)), GOL_FILM=r0,c0,rows,cols)");
    Film out;
    out.n = film_frames();
    out.frames.resize(out.n * (size_t)(film_geo_.rows * film_geo_.cols));
    out.start = film_into(out.frames.data(), out.n);
    return out;
}

size_t Engine::film_frames() {
    if (!cfg_.film.on) throw Error("film(): this engine is not in film mode");
    census_collect();
    return film_host_.size() / (size_t)film_geo_.slot_words();
}

u64 Engine::film_into(u8* out, size_t n) {
    if (!cfg_.film.on) throw Error("film(): this engine is not in film mode");
    const size_t slot = (size_t)film_geo_.slot_words();
    if (n * slot != film_host_.size()) throw Error("film_into(): the record has changed since film_frames()");
    std::vector<u64> sum;
    const u64* packed = film_host_.data();
    if (t_->size() > 1) {  // (every word has one owner: the sum puts the ranks' words side by side)
        sum = film_host_;
        sum_series(sum, "film");
        packed = sum.data();
    }
    const i64 rows = film_geo_.rows, cols = film_geo_.cols, fw = film_geo_.fw, total = (i64)n * rows;
#pragma omp parallel for schedule(static) if (total * cols > 65536)
    for (i64 r = 0; r < total; ++r) film_geo_.unpack_row(packed + r * fw, out + r * cols);
    return census_start_;
}

void Engine::film_clear() {
    if (!cfg_.film.on) throw Error("film_clear(): this engine is not in film mode");
    census_collect();
    census_restart(census_start_ + (u64)(film_host_.size() / (size_t)film_geo_.slot_words()));
}

// ---------------------------------------------------------------------------------------------
// Density film (density-film mode's record: density_host_, this rank's maps; gol/density_film.hpp)
// ---------------------------------------------------------------------------------------------

Engine::DensityFilm Engine::density_film() {
    if (!cfg_.density_film.on)
        throw Error("density_film(): this engine is not in density-film mode (EngineConfig::density_film, "
                    "Simulation(density_film=(block_rows, block_cols)), GOL_DENSITY_FILM=block_rows[,block_cols])");
    DensityFilm out;
    out.n = density_film_frames();
    out.maps.resize(out.n * (size_t)density_geo_.blocks());
    out.start = density_film_into(out.maps.data(), out.n);
    return out;
}

size_t Engine::density_film_frames() {
    if (!cfg_.density_film.on) throw Error("density_film(): this engine is not in density-film mode");
    census_collect();
    return density_host_.size() / (size_t)density_geo_.slot_words();
}

u64 Engine::density_film_into(u32* out, size_t n) {
    if (!cfg_.density_film.on) throw Error("density_film(): this engine is not in density-film mode");
    const size_t slot = (size_t)density_geo_.slot_words(), blocks = (size_t)density_geo_.blocks();
    if (n * slot != density_host_.size()) throw Error("density_film_into(): the record has changed since density_film_frames()");
    // The ranks' maps are summed a few at a time (about 1 MiB of slots per round, one map at least): a block's count
    // is below 2^32, so the two counts of a u64 word add up without a carry between them.
    const size_t per = std::max<size_t>(1, ((size_t)1 << 17) / slot);
    std::vector<u64> part;
    for (size_t at = 0; at < n; at += per) {
        const size_t m = std::min(per, n - at);
        const u64* words = density_host_.data() + at * slot;
        if (t_->size() > 1) {
            part.assign(words, words + m * slot);
            sum_series(part, "density_film");
            words = part.data();
        }
        for (size_t i = 0; i < m; ++i) memcpy(out + (at + i) * blocks, words + i * slot, blocks * sizeof(u32));
    }
    return census_start_;
}

void Engine::density_film_clear() {
    if (!cfg_.density_film.on) throw Error("density_film_clear(): this engine is not in density-film mode");
    census_collect();
    census_restart(census_start_ + (u64)(density_host_.size() / (size_t)density_geo_.slot_words()));
}

// ---------------------------------------------------------------------------------------------
// Envelope (envelope mode: the backends keep E beside the board; the board's readers run on it)
// ---------------------------------------------------------------------------------------------

void Engine::need_envelope(const char* what) const {
    if (!cfg_.envelope)
        throw Error(std::string(what) + ": this engine is not in envelope mode (EngineConfig::envelope, Simulation(envelope=True), GOL_ENVELOPE=1)");
}

void Engine::envelope_reset() {
    env_start_ = gen_;
    stats_.envelope_start = env_start_;
    envelope_merge_local(true);
}

namespace {
struct ViewEnvelope {  // the board's readers read the envelope while this lives
    explicit ViewEnvelope(bool& f) : f_(f) { f_ = true; }
    ~ViewEnvelope() { f_ = false; }
    bool& f_;
};
}  // namespace

u64 Engine::envelope_start() const {
    need_envelope("envelope()");
    return env_start_;
}

std::vector<u64> Engine::envelope_tile_words() {
    need_envelope("envelope()");
    ViewEnvelope v(view_env_);
    return tile_words();
}

std::vector<u8> Engine::envelope_window(i64 r0, i64 c0, i64 rows, i64 cols) {
    need_envelope("envelope_window()");
    ViewEnvelope v(view_env_);
    return window(r0, c0, rows, cols);
}

std::vector<u32> Engine::envelope_density(i64 block_rows, i64 block_cols) {
    need_envelope("envelope_density()");
    ViewEnvelope v(view_env_);
    return density(block_rows, block_cols);
}

u64 Engine::envelope_population() {
    need_envelope("envelope_population()");
    ViewEnvelope v(view_env_);
    return population();
}

void Engine::envelope_clear() {
    need_envelope("envelope_clear()");
    envelope_reset();
}

// ---------------------------------------------------------------------------------------------
// Generations rules (the backends keep 1 + M planes; the board's readers run on each plane)
// ---------------------------------------------------------------------------------------------

void Engine::need_generations(const char* what) const {
    if (!generations())
        throw Error(std::string(what) + ": rule " + cfg_.rule.str() + " has two states; the state calls are for Generations rules "
                    "(B<digits>/S<digits>/C<n>, Simulation(rule=\"B2/S345/C4\"), GOL_RULE=B2/S345/C4)");
}

void Engine::need_two_states(const char* what) const {
    if (generations())
        throw Error(std::string(what) + ": not built for Generations rules in this version (the rule is " + cfg_.rule.str() + ")");
}

void Engine::need_rule_code(const char* what) const {
    if (ltl())
        throw Error(std::string(what) + ": not built for Larger than Life rules in this version (the rule is " + cfg_.rule.str() +
                    "): a checkpoint's header holds Rule::code(), which such a rule does not have");
}

namespace {
struct ViewPlane {  // the board's readers read plane p while this lives
    ViewPlane(int& v, int p) : v_(v) { v_ = p; }
    ~ViewPlane() { v_ = 0; }
    int& v_;
};
}  // namespace

std::vector<u8> Engine::state_window(i64 r0, i64 c0, i64 rows, i64 cols) {
    need_generations("state_window()");
    std::vector<u8> out = window(r0, c0, rows, cols);  // (the checks; state 1)
    // decay plane m adds bit m of d = state - 1: a dying cell ends as 1 + d (no cell is alive and dying)
    std::vector<u8> d(out.size(), 0);
    for (int m = 0; m < cfg_.rule.decay_planes(); ++m) {
        ViewPlane v(view_plane_, m + 1);
        const std::vector<u8> plane = window(r0, c0, rows, cols);
        for (size_t i = 0; i < d.size(); ++i) d[i] = (u8)(d[i] | (plane[i] << m));
    }
    for (size_t i = 0; i < out.size(); ++i)
        if (d[i]) out[i] = (u8)(d[i] + 1);
    return out;
}

std::vector<u8> Engine::state_tile() {
    need_generations("state_tile()");
    const i64 h = L_.h, w = L_.w, nw = L_.nw;
    std::vector<u8> out((size_t)(h * w), 0), d((size_t)(h * w), 0);
    for (int p = 0; p <= cfg_.rule.decay_planes(); ++p) {
        ViewPlane v(view_plane_, p);
        const std::vector<u64> words = tile_words();
        std::vector<u8>& to = p == 0 ? out : d;  // plane 0: state 1; plane p: bit p - 1 of d
        for (i64 r = 0; r < h; ++r)
            for (i64 c = 0; c < w; ++c)
                to[(size_t)(r * w + c)] |= (u8)(((words[(size_t)(r * nw + (c >> 6))] >> (c & 63)) & 1ull) << (p == 0 ? 0 : p - 1));
    }
    for (size_t i = 0; i < out.size(); ++i)
        if (d[i]) out[i] = (u8)(d[i] + 1);
    return out;
}

void Engine::set_state_tile(const std::vector<u8>& states) {
    need_generations("set_state_tile()");
    const i64 h = L_.h, w = L_.w, nw = L_.nw;
    if ((i64)states.size() != h * w)
        throw Error(strprintf("set_state_tile(): %zu states for a tile of %lld x %lld cells", states.size(), (long long)h, (long long)w));
    for (size_t i = 0; i < states.size(); ++i)
        if (states[i] >= cfg_.rule.states)
            throw Error(strprintf("set_state_tile(): state %d at (%lld, %lld): rule %s has the states 0 .. %d", (int)states[i],
                                  (long long)((i64)i / w), (long long)((i64)i % w), cfg_.rule.str().c_str(), (int)cfg_.rule.states - 1));
    const int M = cfg_.rule.decay_planes();
    std::vector<std::vector<u64>> planes((size_t)(M + 1), std::vector<u64>((size_t)(h * nw), 0));
    for (i64 r = 0; r < h; ++r)
        for (i64 c = 0; c < w; ++c) {
            const unsigned s = states[(size_t)(r * w + c)];
            const size_t at = (size_t)(r * nw + (c >> 6));
            if (s == 1) planes[0][at] |= 1ull << (c & 63);
            for (int m = 0; s >= 2 && m < M; ++m)
                if (((s - 1) >> m) & 1u) planes[(size_t)(m + 1)][at] |= 1ull << (c & 63);
        }
    std::vector<const u64*> ptrs;
    for (const auto& p : planes) ptrs.push_back(p.data());
    write_planes_local(ptrs);
}

std::vector<u64> Engine::state_counts() {
    need_generations("state_counts()");
    std::vector<u64> counts((size_t)cfg_.rule.states, 0);
    state_counts_local(counts.data());
    return counts;  // (one rank: the tile is the board)
}

// ---------------------------------------------------------------------------------------------
// Signatures (signature mode's record: census_host_ the populations, sig_host_ the signatures)
// ---------------------------------------------------------------------------------------------

void Engine::sum_series(std::vector<u64>& out, const char* what) {
    if (t_->size() == 1) return;
    const size_t n = out.size();
    std::vector<std::vector<u8>> all;
    t_->gatherv(out.data(), n * sizeof(u64), &all, 0);
    u64 ok = 1;
    if (g_.rank == 0)
        for (int q = 1; q < t_->size(); ++q) {
            if (all[(size_t)q].size() != n * sizeof(u64)) {
                ok = 0;
                break;
            }
            u64 part = 0;
            for (size_t i = 0; i < n; ++i) {
                memcpy(&part, all[(size_t)q].data() + i * sizeof(u64), sizeof(u64));
                out[i] += part;
            }
        }
    t_->broadcast(&ok, sizeof(ok), 0);
    if (!ok) throw Error(std::string(what) + ": the ranks' series differ in length (every rank must run the same generations)");
    if (n > 0) t_->broadcast(out.data(), n * sizeof(u64), 0);
}

Engine::SignatureSeries Engine::signatures() {
    if (!cfg_.signature)
        throw Error("signatures(): this engine is not in signature mode (EngineConfig::signature, Simulation(signature=True), GOL_SIGNATURE=1)");
    census_collect();
    SignatureSeries s;
    s.start = census_start_;
    s.signatures = sig_host_;
    s.populations = census_host_;
    sum_series(s.signatures, "signatures");
    sum_series(s.populations, "signatures");
    return s;
}

void Engine::signatures_clear() {
    if (!cfg_.signature) throw Error("signatures_clear(): this engine is not in signature mode");
    census_collect();
    census_restart(census_start_ + (u64)census_host_.size());
}

u64 Engine::signature() { return t_->allreduce_sum(local_signature()); }

void Engine::snapshot() {
    snapshot_local();
    have_snapshot_ = true;
}

u64 Engine::snapshot_diff() {
    if (!have_snapshot_) throw Error("snapshot_diff(): no snapshot has been taken since init (call snapshot() first)");
    return t_->allreduce_sum(snapshot_diff_local());
}

// ---------------------------------------------------------------------------------------------
// Views and pattern stamping (collective wrappers; the backends do the rank-local part)
// ---------------------------------------------------------------------------------------------

StampMode parse_stamp_mode(const std::string& s) {
    if (s == "or") return StampMode::Or;
    if (s == "replace") return StampMode::Replace;
    if (s == "xor") return StampMode::Xor;
    if (s == "clear") return StampMode::Clear;
    throw Error("stamp mode must be or, replace, xor or clear (got '" + s + "')");
}

std::vector<Engine::Piece> Engine::pieces(const Geometry& g, i64 r0, i64 c0, i64 rows, i64 cols) {
    // the rectangle cut at the seams: up to two row spans x two column spans of the global board
    struct Span {
        i64 at, n, off;  // global start, length, offset inside the rectangle
    };
    auto spans = [](i64 start, i64 n, i64 size) {
        const i64 s = pmod(start, size);
        std::vector<Span> v;
        const i64 first = std::min(n, size - s);
        v.push_back({s, first, 0});
        if (n > first) v.push_back({0, n - first, first});
        return v;
    };
    std::vector<Piece> out;
    for (const Span& rs : spans(r0, rows, g.dec.H))
        for (const Span& cs : spans(c0, cols, g.dec.W)) {
            const i64 ra = std::max(rs.at, g.row0), rb = std::min(rs.at + rs.n, g.row0 + g.h);
            const i64 ca = std::max(cs.at, g.col0), cb = std::min(cs.at + cs.n, g.col0 + g.w);
            if (ra >= rb || ca >= cb) continue;
            out.push_back({ra - g.row0, ca - g.col0, rb - ra, cb - ca, rs.off + (ra - rs.at), cs.off + (ca - cs.at)});
        }
    return out;
}

void Engine::check_window(i64 rows, i64 cols) const {
    if (rows < 1 || cols < 1 || rows > g_.dec.H || cols > g_.dec.W)
        throw Error(strprintf("window of %lld x %lld cells: rows must be in 1..%lld and columns in 1..%lld (the board)",
                              (long long)rows, (long long)cols, (long long)g_.dec.H, (long long)g_.dec.W));
}

void Engine::check_window(i64 r0, i64 c0, i64 rows, i64 cols) const {
    check_window(rows, cols);
    if (dead_edges() && (r0 < 0 || c0 < 0 || r0 + rows > g_.dec.H || c0 + cols > g_.dec.W))
        throw Error(strprintf("window of %lld x %lld cells at (%lld, %lld) does not lie inside the bounded %lld x %lld board "
                              "(boundary dead: nothing wraps)",
                              (long long)rows, (long long)cols, (long long)r0, (long long)c0, (long long)g_.dec.H,
                              (long long)g_.dec.W));
}

void Engine::check_density(i64 block_rows, i64 block_cols) const {
    if (block_rows < 1) throw Error(strprintf("density: block_rows must be >= 1 (got %lld)", (long long)block_rows));
    if (block_cols < 64 || block_cols % 64 != 0)
        throw Error(strprintf("density: block_cols must be a multiple of 64, the cells of a board word (got %lld)",
                              (long long)block_cols));
    if (std::min(block_rows, g_.dec.H) > (i64)0xFFFFFFFFll / std::min(block_cols, round_up(g_.dec.W, 64)))
        throw Error("density: a block holds more than 2^32 - 1 cells, its count would not fit");
}

void Engine::check_stamp(const RlePattern& p, i64 r0, i64 c0) const {
    check_stamp(p);
    if (dead_edges() && (r0 < 0 || c0 < 0 || r0 + p.rows > g_.dec.H || c0 + p.cols > g_.dec.W))
        throw Error(strprintf("stamp: the pattern (%lld x %lld) at (%lld, %lld) does not lie inside the bounded %lld x %lld "
                              "board (boundary dead: nothing wraps)",
                              (long long)p.rows, (long long)p.cols, (long long)r0, (long long)c0, (long long)g_.dec.H,
                              (long long)g_.dec.W));
}

void Engine::check_stamp(const RlePattern& p) const {
    if (p.rows < 1 || p.cols < 1 || (i64)p.words.size() != p.rows * p.nw())
        throw Error(strprintf("stamp: malformed pattern (%lld x %lld cells, %zu words)", (long long)p.rows,
                              (long long)p.cols, p.words.size()));
    if (p.rows > g_.dec.H || p.cols > g_.dec.W)
        throw Error(strprintf("stamp: the pattern (%lld x %lld) is larger than the board (%lld x %lld) and would overlap "
                              "itself on the torus",
                              (long long)p.rows, (long long)p.cols, (long long)g_.dec.H, (long long)g_.dec.W));
    if (cfg_.compat)
        throw Error("stamp: refused in compat mode (GOL_COMPAT=reference), whose halos are frozen at generation 0");
}

std::vector<u8> Engine::window(i64 r0, i64 c0, i64 rows, i64 cols) {
    check_window(r0, c0, rows, cols);
    std::vector<u8> out((size_t)(rows * cols), 0);
    read_window_local(r0, c0, rows, cols, out.data(), cols);
    if (t_->size() == 1) return out;
    // every rank's pieces follow from the geometry: a rank sends the bytes of its pieces alone, in order
    auto pack = [&](const std::vector<Piece>& ps, std::vector<u8>& bytes, bool unpack) {
        size_t at = 0;
        for (const Piece& p : ps)
            for (i64 r = 0; r < p.rows; ++r, at += (size_t)p.cols) {
                u8* w = &out[(size_t)((p.wr + r) * cols + p.wc)];
                if (unpack)
                    memcpy(w, &bytes[at], (size_t)p.cols);
                else
                    memcpy(&bytes[at], w, (size_t)p.cols);
            }
    };
    auto bytes_of = [](const std::vector<Piece>& ps) {
        size_t n = 0;
        for (const Piece& p : ps) n += (size_t)(p.rows * p.cols);
        return n;
    };
    const std::vector<Piece> mine = pieces(g_, r0, c0, rows, cols);
    std::vector<u8> send(bytes_of(mine));
    pack(mine, send, false);
    std::vector<std::vector<u8>> all;
    t_->gatherv(send.data(), send.size(), &all, 0);
    if (g_.rank == 0)
        for (int q = 1; q < t_->size(); ++q) {
            const std::vector<Piece> ps = pieces(make_geometry(g_.dec, q), r0, c0, rows, cols);
            if (all[(size_t)q].size() != bytes_of(ps)) throw Error(strprintf("window: rank %d sent a part of the wrong size", q));
            pack(ps, all[(size_t)q], true);
        }
    t_->broadcast(out.data(), out.size(), 0);
    return out;
}

std::vector<u32> Engine::density(i64 block_rows, i64 block_cols) {
    check_density(block_rows, block_cols);
    const size_t n = (size_t)(ceil_div(g_.dec.H, block_rows) * ceil_div(g_.dec.W, block_cols));
    std::vector<u32> out(n, 0);
    density_local(block_rows, block_cols, out.data());
    if (t_->size() == 1) return out;
    std::vector<std::vector<u8>> all;
    t_->gatherv(out.data(), n * sizeof(u32), &all, 0);
    if (g_.rank == 0)
        for (int q = 1; q < t_->size(); ++q) {
            if (all[(size_t)q].size() != n * sizeof(u32)) throw Error(strprintf("density: rank %d sent a grid of the wrong size", q));
            const u32* part = reinterpret_cast<const u32*>(all[(size_t)q].data());
            for (size_t i = 0; i < n; ++i) out[i] += part[i];
        }
    t_->broadcast(out.data(), n * sizeof(u32), 0);
    return out;
}

void Engine::stamp(const RlePattern& p, i64 r0, i64 c0, StampMode mode) {
    check_stamp(p, r0, c0);
    stamp_local(p, r0, c0, mode);
    if (cfg_.envelope) envelope_merge_local(false);  // E |= board: what the stamp removed stays in E
    if (generations()) settle_decay_local();         // a stamped live cell is not dying as well
}

// ---------------------------------------------------------------------------------------------
// Dense cells: the tensor readers and writers (gol/cells.hpp; the backends convert)
// ---------------------------------------------------------------------------------------------

namespace {
void need_cells(const CellBuffer& b, i64 cells, const char* what) {
    if (b.numel != cells)
        throw Error(strprintf("%s: the buffer holds %lld elements, the cells are %lld", what, (long long)b.numel, (long long)cells));
}
}  // namespace

CellSource Engine::tile_source(const u64* buf, i64 r0, i64 c0, i64 rows, i64 cols) const {
    CellSource s;
    s.base = buf + L_.index(0, 0);
    s.words = L_.words() - L_.index(0, 0);
    s.frame_stride = 0, s.row_stride = L_.pitch;
    s.n = 1, s.rows = rows, s.cols = cols;
    s.r0 = pmod(r0, L_.h), s.H = L_.h;
    s.c0 = pmod(c0, L_.w), s.W = L_.w;
    s.w0 = 0, s.gwords = L_.nw, s.fw = L_.nw;
    return s;
}

CellSource Engine::film_source(const u64* frames, i64 words, i64 n) const {
    const FilmGeo& f = film_geo_;
    CellSource s;
    s.base = frames;
    s.words = words;
    s.frame_stride = f.slot_words(), s.row_stride = f.fw;
    s.n = n, s.rows = f.rows, s.cols = f.cols;
    s.r0 = 0, s.H = f.rows;
    s.c0 = f.c0, s.W = f.W;
    s.w0 = f.w0, s.gwords = f.gwords, s.fw = f.fw;
    return s;
}

void Engine::read_tile_cells(const CellBuffer& dst) {
    need_two_states("read_tile_cells()");
    need_cells(dst, L_.h * L_.w, "read_tile_cells()");
    check_cell_pointer(dst, "read_tile_cells()");
    read_rect_cells(0, 0, L_.h, L_.w, dst);
}

void Engine::read_envelope_cells(const CellBuffer& dst) {
    need_envelope("read_envelope_cells()");
    need_cells(dst, L_.h * L_.w, "read_envelope_cells()");
    check_cell_pointer(dst, "read_envelope_cells()");
    ViewEnvelope v(view_env_);
    read_rect_cells(0, 0, L_.h, L_.w, dst);
}

void Engine::write_tile_cells(const CellBuffer& src) {
    need_two_states("write_tile_cells()");
    need_cells(src, L_.h * L_.w, "write_tile_cells()");
    check_cell_pointer(src, "write_tile_cells()");
    write_tile_cells_local(src);
    if (cfg_.envelope) envelope_reset();
}

void Engine::read_window_cells(i64 r0, i64 c0, i64 rows, i64 cols, const CellBuffer& dst) {
    need_two_states("read_window_cells()");
    if (t_->size() > 1)
        throw Error(strprintf("read_window_cells(): this job has %d ranks; a window is unpacked on the device for one rank "
                              "only (use window())", t_->size()));
    check_window(r0, c0, rows, cols);
    need_cells(dst, rows * cols, "read_window_cells()");
    check_cell_pointer(dst, "read_window_cells()");
    read_rect_cells(r0, c0, rows, cols, dst);  // (one rank: the tile is the board)
}

void Engine::run_film_cells(u64 generations, const CellBuffer& dst) {
    if (!cfg_.film.on)
        throw Error("run_film_cells(): this engine is not in film mode (EngineConfig::film, Simulation(film=(r0, c0, rows, cols)), GOL_FILM=r0,c0,rows,cols)");
    if (t_->size() > 1)
        throw Error(strprintf("run_film_cells(): this job has %d ranks; frames are unpacked on the device for one rank only "
                              "(use run() and film())", t_->size()));
    const size_t held = film_frames();
    if (held != 0)
        throw Error(strprintf("run_film_cells(): the film record holds %zu frames; call film_clear() first", held));
    const i64 per = film_geo_.rows * film_geo_.cols;
    if (generations > (u64)(((i64)1 << 52) / per)) throw Error("run_film_cells(): more than 2^52 cells");
    need_cells(dst, (i64)generations * per, "run_film_cells()");
    if (generations > 0) check_cell_pointer(dst, "run_film_cells()");
    for (u64 done = 0; done < generations;) {
        const u64 n = std::min<u64>(generations - done, film_chunk());
        run(n);
        film_drain_cells((size_t)n, dst, (size_t)done);
        done += n;
    }
    census_restart(gen_);
}

// ---------------------------------------------------------------------------------------------
// Pattern matching (gol/match.hpp; the backends run the matcher)
// ---------------------------------------------------------------------------------------------

void Engine::check_match(const std::vector<std::pair<int, MatchTemplate>>& ts, const char* what) const {
    if (t_->size() > 1)
        throw Error(strprintf("%s: this job has %d ranks; matching is built for one rank (a tile's edge cells need the "
                              "neighbours' rows)", what, t_->size()));
    if (ts.empty()) throw Error(std::string(what) + ": no template");
    for (const auto& e : ts) {
        if (e.first < 0 || e.first > 7) throw Error(strprintf("%s: orientation id %d is outside 0 .. 7", what, e.first));
        e.second.validate(g_.dec.H, g_.dec.W);
    }
}

Engine::MatchResult Engine::match(const std::vector<std::pair<int, MatchTemplate>>& ts, i64 max_hits, bool positions) {
    check_match(ts, "match()");
    if (max_hits < 1) throw Error(strprintf("match(): max_hits = %lld is less than 1", (long long)max_hits));
    MatchResult res;
    std::vector<i32> pos;
    std::vector<u8> ids;
    for (const auto& e : ts) {  // one bitmap, reused: match, read the count, compact, then the next orientation
        const u64 n = match_local(e.second, positions, false);
        stats_.match_launches += 1;
        res.count += n;
        const i64 room = max_hits - (i64)ids.size();
        if (!positions || n == 0 || room <= 0) continue;
        const i64 take = (i64)std::min<u64>(n, (u64)room);
        match_positions_local(take, &pos);
        ids.resize(ids.size() + (size_t)take, (u8)e.first);
    }
    res.truncated = res.count > (u64)max_hits;
    if (!positions) return res;
    std::vector<size_t> order(ids.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (pos[2 * a] != pos[2 * b]) return pos[2 * a] < pos[2 * b];
        if (pos[2 * a + 1] != pos[2 * b + 1]) return pos[2 * a + 1] < pos[2 * b + 1];
        return ids[a] < ids[b];
    });
    res.positions.reserve(pos.size());
    res.orientation.reserve(ids.size());
    for (size_t i : order) {
        res.positions.push_back(pos[2 * i]);
        res.positions.push_back(pos[2 * i + 1]);
        res.orientation.push_back(ids[i]);
    }
    return res;
}

void Engine::match_cells(const std::vector<std::pair<int, MatchTemplate>>& ts, const CellBuffer& dst) {
    need_two_states("match_cells()");
    check_match(ts, "match_cells()");
    need_cells(dst, L_.h * L_.w, "match_cells()");
    check_cell_pointer(dst, "match_cells()");
    for (size_t i = 0; i < ts.size(); ++i) {
        match_local(ts[i].second, true, i > 0);
        stats_.match_launches += 1;
    }
    match_bitmap_cells(dst);
}

// ---------------------------------------------------------------------------------------------
// Connected components (gol/components.hpp; the backends label)
// ---------------------------------------------------------------------------------------------

void Engine::check_components(i64 max_objects, const char* what) const {
    if (t_->size() > 1)
        throw Error(strprintf("%s: this job has %d ranks; components are built for one rank (an object may cross a tile's "
                              "edge)", what, t_->size()));
    cc_check(g_.dec.H, g_.dec.W, 1, max_objects, what);
}

ComponentsResult Engine::components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) {
    check_components(max_objects, "components()");
    return components_local(nb, max_objects, hashes, want_records);
}

void Engine::components_labels(CcNeighbourhood nb, void* dst, bool int64, i64 numel) {
    check_components(1, "components_labels()");
    if (numel != L_.h * L_.w)
        throw Error(strprintf("components_labels(): the buffer holds %lld elements, the board %lld x %lld cells", (long long)numel,
                              (long long)L_.h, (long long)L_.w));
    const i64 size = int64 ? 8 : 4;
    if (!dst || reinterpret_cast<uintptr_t>(dst) % (uintptr_t)size) throw Error("components_labels(): the buffer is not aligned to its element");
    check_cell_pointer(CellBuffer{dst, CellType::U8, numel * size}, "components_labels()");
    components_labels_cells(nb, dst, int64);
}

// ---------------------------------------------------------------------------------------------
// CPU backend
// ---------------------------------------------------------------------------------------------

namespace {

class CpuEngine : public Engine {
   public:
    CpuEngine(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t) : Engine(g, c, std::move(t)) {
        planes_ = 1 + cfg_.rule.decay_planes();  // (a Generations rule: the decay planes follow the live plane)
        a_.assign((size_t)(planes_ * L_.words()), 0);
        b_.assign((size_t)(planes_ * L_.words()), 0);
        if (cfg_.envelope) env_.assign((size_t)L_.words(), 0);
        cur_ = a_.data();
        oth_ = b_.data();
    }
    std::string backend_name() const override { return "cpu"; }
    void synchronize() override {}

    std::vector<u64> tile_words() override {
        std::vector<u64> d((size_t)(L_.h * L_.nw));
        cpu::extract_words(view_buf(), L_, d.data());
        return d;
    }
    void set_tile_words(const std::vector<u64>& dense) override {
        if ((i64)dense.size() != L_.h * L_.nw) throw Error("set_tile_words: wrong size");
        write_planes_local({dense.data()});
        if (cfg_.envelope) envelope_reset();
    }
    // the live plane, then the decay planes (a plane that is not given: zeros)
    void write_planes_local(const std::vector<const u64*>& planes) override {
        const std::vector<u64> zeros((size_t)(L_.h * L_.nw), 0);
        for (i64 p = 0; p < planes_; ++p)
            cpu::insert_words(cur_ + p * L_.words(), L_, (size_t)p < planes.size() && planes[(size_t)p] ? planes[(size_t)p] : zeros.data());
        refresh_local(cur_);
    }
    void settle_decay_local() override {
        for (i64 p = 1; p < planes_; ++p)
            for (i64 r = 0; r < L_.h; ++r)
                for (i64 c = 0; c < L_.nw; ++c) cur_[p * L_.words() + L_.index(r, c)] &= ~cur_[L_.index(r, c)];
        refresh_local(cur_);
    }
    void state_counts_local(u64* counts) override { cpu::state_counts(cur_, L_, L_.words(), cfg_.rule, counts); }
    std::pair<u64, u64> local_reduce() override {
        return {cpu::population(view_buf(), L_),
                cpu::fingerprint(view_buf(), L_, g_.row0, g_.word0(), g_.global_words())};
    }
    // E = (reset ? 0 : E) | the tile's own cells (ghost rows and words of E stay 0)
    void envelope_merge_local(bool reset) override {
        if (reset) std::fill(env_.begin(), env_.end(), 0);
        cpu::envelope_or(env_.data(), cur_, L_);
    }
    u64 local_signature() override { return cpu::signature(cur_, L_, g_.row0, g_.word0()); }
    void snapshot_local() override { snap_.assign(cur_, cur_ + L_.words()); }
    u64 snapshot_diff_local() override {
        u64 n = 0;
        for (i64 r = 0; r < L_.h; ++r) {
            const u64 *a = cur_ + L_.index(r, 0), *b = snap_.data() + L_.index(r, 0);
            for (i64 c = 0; c < L_.nw; ++c) n += (u64)__builtin_popcountll((a[c] ^ b[c]) & storage_mask(c, L_.w));
        }
        return n;
    }

    void read_window_local(i64 r0, i64 c0, i64 rows, i64 cols, u8* out, i64 stride) override {
        check_window(r0, c0, rows, cols);
        for (const Piece& p : pieces(g_, r0, c0, rows, cols))
            for (i64 r = 0; r < p.rows; ++r) {
                const u64* row = view_buf() + L_.index(p.tr + r, 0);
                u8* o = out + (p.wr + r) * stride + p.wc;
                for (i64 c = 0; c < p.cols; ++c) {
                    const i64 tc = p.tc + c;
                    o[c] = (u8)(((merge_word(row[tc >> 6]) & L_.mask(tc >> 6)) >> (tc & 63)) & 1ull);
                }
            }
    }

    void density_local(i64 block_rows, i64 block_cols, u32* counts) override {
        check_density(block_rows, block_cols);
        const i64 gcols = ceil_div(g_.dec.W, block_cols), wpb = block_cols / 64;
        for (i64 r = 0; r < L_.h; ++r) {
            const u64* row = view_buf() + L_.index(r, 0);
            u32* line = counts + ((g_.row0 + r) / block_rows) * gcols;
            for (i64 c = 0; c < L_.nw; ++c)
                line[(g_.word0() + c) / wpb] += (u32)__builtin_popcountll(row[c] & storage_mask(c, L_.w));
        }
    }

    void stamp_local(const RlePattern& p, i64 r0, i64 c0, StampMode mode) override {
        check_stamp(p, r0, c0);
        for (const Piece& q : pieces(g_, r0, c0, p.rows, p.cols))
            for (i64 r = 0; r < q.rows; ++r) {
                u64* row = cur_ + L_.index(q.tr + r, 0);
                const u64* prow = &p.words[(size_t)((q.wr + r) * p.nw())];
                for (i64 cw = q.tc >> 6; cw <= (q.tc + q.cols - 1) >> 6; ++cw)
                    row[cw] = stamp_word(row[cw], prow, q.wc, q.tc, q.cols, cw, (int)mode);
            }
        refresh_local(cur_);
    }

   protected:
    // dense cells: host memory, host loops (gol/cells.hpp)
    void check_cell_pointer(const CellBuffer&, const char*) override {}
    void read_rect_cells(i64 r0, i64 c0, i64 rows, i64 cols, const CellBuffer& dst) override {
        unpack_cells_host(tile_source(view_buf(), r0, c0, rows, cols), dst);
    }
    void write_tile_cells_local(const CellBuffer& src) override {
        CellTarget t;
        t.base = cur_ + L_.index(0, 0);
        t.words = L_.words() - L_.index(0, 0);
        t.row_stride = L_.pitch, t.rows = L_.h, t.cols = L_.w;
        pack_cells_host(src, t);
        refresh_local(cur_);
    }
    // pattern matching: the host matcher on the board's natural-order words; the bitmap stays in natural order
    u64 match_local(const MatchTemplate& t, bool keep, bool or_into) override {
        std::vector<u64> d((size_t)(L_.h * L_.nw));
        cpu::extract_words(cur_, L_, d.data());
        if (keep) match_bits_.resize(d.size(), 0);
        return match_host(d.data(), L_.h, L_.w, !dead_edges(), t, keep ? match_bits_.data() : nullptr, or_into);
    }
    void match_positions_local(i64 cap, std::vector<i32>* out) override {
        match_positions_host(match_bits_.data(), L_.h, L_.w, cap, out);
    }
    void match_bitmap_cells(const CellBuffer& dst) override {
        std::vector<u64> split(match_bits_.size());
        for (size_t i = 0; i < split.size(); ++i) split[i] = split_word(match_bits_[i]);
        CellSource s;
        s.base = split.data();
        s.words = (i64)split.size();
        s.frame_stride = 0, s.row_stride = L_.nw;
        s.n = 1, s.rows = L_.h, s.cols = L_.w;
        s.r0 = 0, s.H = L_.h;
        s.c0 = 0, s.W = L_.w;
        s.w0 = 0, s.gwords = L_.nw, s.fw = L_.nw;
        unpack_cells_host(s, dst);
    }
    // connected components: the host labeller on the board's natural-order words
    ComponentsResult components_local(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) override {
        std::vector<u64> d((size_t)(L_.h * L_.nw));
        cpu::extract_words(cur_, L_, d.data());
        return components_host(d.data(), L_.h, L_.w, 1, !dead_edges(), nb, max_objects, hashes, want_records, nullptr);
    }
    void components_labels_cells(CcNeighbourhood nb, void* dst, bool int64) override {
        std::vector<u64> d((size_t)(L_.h * L_.nw));
        cpu::extract_words(cur_, L_, d.data());
        std::vector<i32> lab((size_t)(L_.h * L_.w));
        components_host(d.data(), L_.h, L_.w, 1, !dead_edges(), nb, 1, false, false, lab.data());
        if (int64)
            std::copy(lab.begin(), lab.end(), static_cast<i64*>(dst));
        else
            std::copy(lab.begin(), lab.end(), static_cast<i32*>(dst));
    }
    size_t film_chunk() const override {  // (the host record between two drains stays below 64 MiB)
        return std::max<size_t>(8, ((size_t)64 << 20) / ((size_t)film_geo_.slot_words() * sizeof(u64)));
    }
    void film_drain_cells(size_t frames, const CellBuffer& dst, size_t at) override {
        const i64 per = film_geo_.rows * film_geo_.cols;
        if (film_host_.size() != frames * (size_t)film_geo_.slot_words()) throw Error("run_film_cells(): the record is not the chunk's");
        CellBuffer part{(u8*)dst.ptr + at * (size_t)(per * cell_size(dst.type)), dst.type, (i64)frames * per};
        unpack_cells_host(film_source(film_host_.data(), (i64)film_host_.size(), (i64)frames), part);
        film_host_.clear();
    }

    void do_init(const PatternSpec& p) override {
        cpu::init_tile(cur_, L_, g_, p);
        std::fill(cur_ + L_.words(), cur_ + planes_ * L_.words(), 0);  // (the decay planes: nothing is dying)
        std::fill(oth_, oth_ + planes_ * L_.words(), 0);
        refresh_local(cur_);
    }

    void refresh_local(u64* buf) {
        for (i64 p = 0; p < planes_; ++p) {
            if (self_x()) cpu::fill_ghost_cols_wrap(buf + p * L_.words(), L_, 0, L_.h);
            if (self_y() && !cfg_.compat) cpu::fill_ghost_rows_wrap(buf + p * L_.words(), L_);
        }
    }

    void exchange(int k) {
        std::vector<HaloItem> items = halo_items(k);
        if (items.empty()) return;
        std::vector<Message> sends, recvs;
        stage_s_.resize(items.size());
        stage_r_.resize(items.size());
        for (size_t i = 0; i < items.size(); ++i) {
            const HaloItem& it = items[i];
            if (it.contiguous) {
                sends.push_back({it.send_peer, cur_ + L_.index(it.send.r0, it.send.c0), (size_t)it.send.count() * 8});
                recvs.push_back({it.recv_peer, cur_ + L_.index(it.recv.r0, it.recv.c0), (size_t)it.recv.count() * 8});
            } else {
                stage_s_[i].resize((size_t)it.send.count());
                stage_r_[i].resize((size_t)it.recv.count());
                for (i64 r = 0; r < it.send.rows; ++r)
                    memcpy(&stage_s_[i][(size_t)(r * it.send.words)], cur_ + L_.index(it.send.r0 + r, it.send.c0),
                           (size_t)it.send.words * 8);
                sends.push_back({it.send_peer, stage_s_[i].data(), stage_s_[i].size() * 8});
                recvs.push_back({it.recv_peer, stage_r_[i].data(), stage_r_[i].size() * 8});
            }
            stats_.halo_bytes += (u64)it.send.count() * 8;
        }
        t_->exchange_host(sends, recvs);
        for (size_t i = 0; i < items.size(); ++i) {
            const HaloItem& it = items[i];
            if (it.contiguous) continue;
            for (i64 r = 0; r < it.recv.rows; ++r)
                memcpy(cur_ + L_.index(it.recv.r0 + r, it.recv.c0), &stage_r_[i][(size_t)(r * it.recv.words)],
                       (size_t)it.recv.words * 8);
        }
        stats_.exchanges += 1;
    }

    void do_superstep(int k) override {
        if (!cfg_.compat) {
            exchange(k);
            if (self_y())
                for (i64 p = 0; p < planes_; ++p) cpu::fill_ghost_rows_wrap(cur_ + p * L_.words(), L_);
        }
        u64 *counts = nullptr, *sigs = nullptr;
        if (cfg_.census || cfg_.signature) {  // this rank's own cells after each of the k generations
            census_host_.resize(census_host_.size() + (size_t)k, 0);
            counts = census_host_.data() + (census_host_.size() - (size_t)k);
        }
        if (cfg_.signature) {
            sig_host_.resize(sig_host_.size() + (size_t)k, 0);
            sigs = sig_host_.data() + (sig_host_.size() - (size_t)k);
        }
        cpu::Edges place(cfg_.boundary, g_);  // (the signature's keys need the tile's place on the torus too)
        cpu::FilmOut film;
        if (cfg_.film.on) {  // this rank's words of the window after each of the k generations
            const size_t add = (size_t)k * (size_t)film_geo_.slot_words();
            film_host_.resize(film_host_.size() + add, 0);
            film = cpu::FilmOut{&film_geo_, film_host_.data() + (film_host_.size() - add)};
        }
        cpu::DensityOut dens;
        if (cfg_.density_film.on) {  // this rank's counts of every block after each of the k generations
            const size_t add = (size_t)k * (size_t)density_geo_.slot_words();
            density_host_.resize(density_host_.size() + add, 0);
            dens = cpu::DensityOut{&density_geo_, density_host_.data() + (density_host_.size() - add)};
        }
        u64* res = cpu::superstep(cur_, oth_, L_, k, cfg_.rule, place, counts, sigs, film, dens,
                                  cfg_.envelope ? env_.data() : nullptr, L_.words());
        if (res != cur_) std::swap(cur_, oth_);
        if (self_x())
            for (i64 p = 0; p < planes_; ++p) cpu::fill_ghost_cols_wrap(cur_ + p * L_.words(), L_, 0, L_.h);
    }

    void do_set_compat_halos(const std::vector<u64>& above, const std::vector<u64>& below) override {
        for (u64* buf : {a_.data(), b_.data()}) {
            memcpy(buf + L_.index(-1, -1), above.data(), (size_t)L_.pitch * 8);
            memcpy(buf + L_.index(L_.h, -1), below.data(), (size_t)L_.pitch * 8);
            if (self_x()) {
                cpu::fill_ghost_cols_wrap(buf, L_, -1, 0);
                cpu::fill_ghost_cols_wrap(buf, L_, L_.h, L_.h + 1);
            }
        }
    }

    std::vector<u64> read_row(i64 r) override {
        return std::vector<u64>(cur_ + L_.index(r, -1), cur_ + L_.index(r, -1) + L_.pitch);
    }

   private:
    const u64* view_buf() const { return view_env_ ? env_.data() : cur_ + view_plane_ * L_.words(); }
    i64 planes_ = 1;  // 1 + M under a Generations rule: a_ and b_ hold that many boards, L_.words() apart
    std::vector<u64> a_, b_, snap_;
    std::vector<u64> env_;  // envelope mode: E in the board's layout
    std::vector<u64> match_bits_;  // match(): the last bitmap, h x nw natural-order words
    u64* cur_;
    u64* oth_;
    std::vector<std::vector<u64>> stage_s_, stage_r_;
};

}  // namespace

std::unique_ptr<Engine> make_cpu_engine(const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t) {
    return std::make_unique<CpuEngine>(g, c, std::move(t));
}

}  // namespace gol
