// gol-mi355x: soup batches (soups.hpp) -- what both backends share (validation, the launch loops, records and board
// fetches) and the CPU backend: the per-soup program of step_soups on packed split-format words, one soup per OpenMP
// iteration.
#include <algorithm>
#include <cstring>

#include "gol/bits.hpp"
#include "gol/soups.hpp"

namespace gol {

// ---- shared ---------------------------------------------------------------------------------------------------

void SoupBatch::validate(const SoupConfig& c) {
    if (c.size != 64 && c.size != 128 && c.size != 256)
        throw Error(strprintf("soups: size %lld is not supported (a soup is a square torus of side 64, 128 or 256)",
                              (long long)c.size));
    if (c.n < 1 || c.n > kSoupsMax)
        throw Error(strprintf("soups: n = %lld is outside 1 .. 2^20", (long long)c.n));
    if (c.rule.generations())
        throw Error("soups: rule " + c.rule.str() + " is a Generations rule; soup batches run two-state rules only in this version");
    if (c.rule.ltl())
        throw Error("soups: rule " + c.rule.str() + " is a Larger than Life rule; soup batches run radius-1 rules only in this version");
    if (c.rule.nbhd != Nbhd::Moore)
        throw Error("soups: rule " + c.rule.str() + " counts the " + nbhd_name(c.rule.nbhd) +
                    " neighbourhood; soup batches run Moore rules only");
    if (c.boundary != "torus")
        throw Error("soups: boundary \"" + c.boundary + "\" is refused; a soup is a torus");
    if (c.compat) throw Error("soups: compat mode (GOL_COMPAT=reference) is refused; a soup is a correct torus");
    if (c.backend != "hip" && c.backend != "cpu")
        throw Error("soups: backend must be hip or cpu (got " + c.backend + ")");
    if (c.workgroup != 0 && c.workgroup != 64 && c.workgroup != 128 && c.workgroup != 256)
        throw Error(strprintf("soups: workgroup %d is not 64, 128 or 256", c.workgroup));
}

std::unique_ptr<SoupBatch> SoupBatch::create(const SoupConfig& c) {
    validate(c);
    return c.backend == "cpu" ? make_cpu_soups(c) : make_hip_soups(c);
}

void SoupBatch::init_seed(u64 seed) {
    do_init_seed(seed);
    searching_ = false;
    reached_ = launches_ = settled_ = 0;
}

void SoupBatch::init_words(const u64* natural) {
    const size_t total = (size_t)(cfg_.n * words_per_soup());
    std::vector<u64> split(total);
#pragma omp parallel for schedule(static) if (total > 65536)
    for (size_t i = 0; i < total; ++i) split[i] = split_word(natural[i]);
    do_upload(split.data());
    searching_ = false;
    reached_ = launches_ = settled_ = 0;
}

void SoupBatch::step(u64 g) {
    if (searching_)
        throw Error("soups: step() after settle(): the settled soups stand at different generations");
    if (reached_ + g > kSoupMaxGens)
        throw Error(strprintf("soups: step(%llu) from generation %llu passes 2^31", (unsigned long long)g,
                              (unsigned long long)reached_));
    // (one launch per kSoupDefaultChunk generations: no kernel runs unbounded)
    while (g > 0) {
        const u32 now = (u32)std::min<u64>(g, (u64)kSoupDefaultChunk);
        do_plain(now);
        ++launches_;
        reached_ += now;
        g -= now;
    }
}

void SoupBatch::settle(u64 max_gens, bool transient, i64 chunk) {
    if (chunk < 1) throw Error(strprintf("soups: chunk = %lld is below 1", (long long)chunk));
    if (max_gens > kSoupMaxGens)
        throw Error(strprintf("soups: max_gens = %llu is above 2^31", (unsigned long long)max_gens));
    if (max_gens < reached_)
        throw Error(strprintf("soups: max_gens = %llu is below generation %llu, where the soups stand",
                              (unsigned long long)max_gens, (unsigned long long)reached_));
    const u32 budget = (u32)std::min<i64>(chunk, (i64)kSoupMaxGens);
    if (!searching_) {
        do_begin_search();
        searching_ = true;
    }
    while (reached_ < max_gens && settled_ < (u64)cfg_.n) {
        const u32 now = (u32)std::min<u64>(budget, max_gens - reached_);
        settled_ = do_settle(now, (u32)max_gens);
        ++launches_;
        reached_ += now;
    }
    if (transient) {
        // every launch takes a soup `budget` steps further, and a transient is below the generation of the hit
        for (u64 left = settled_; left > 0; ++launches_) left = do_transient(budget);
    }
}

std::vector<SoupRecord> SoupBatch::records() {
    std::vector<SoupState> st((size_t)cfg_.n);
    do_fetch_states(st.data());
    std::vector<SoupRecord> out((size_t)cfg_.n);
    for (size_t i = 0; i < st.size(); ++i) {
        out[i].period = st[i].period;
        out[i].generation = st[i].g;
        out[i].population = st[i].population;
        out[i].transient = (st[i].flags & kSoupTransientDone) ? (i64)st[i].tcount : -1;
    }
    return out;
}

std::vector<u8> SoupBatch::boards(const std::vector<i64>& idx) {
    for (i64 i : idx)
        if (i < 0 || i >= cfg_.n)
            throw Error(strprintf("soups: boards(): index %lld is outside 0 .. %lld", (long long)i, (long long)cfg_.n - 1));
    const i64 S = cfg_.size, M = m(), wps = words_per_soup();
    std::vector<u64> words((size_t)wps * idx.size());
    for (size_t k = 0; k < idx.size(); ++k) do_fetch_board(idx[k], words.data() + k * (size_t)wps);
    std::vector<u8> out((size_t)(S * S) * idx.size());
    const i64 rows = (i64)idx.size() * S;
#pragma omp parallel for schedule(static) if (rows * S > 65536)
    for (i64 r = 0; r < rows; ++r) {
        u8* o = out.data() + (size_t)(r * S);
        for (i64 j = 0; j < M; ++j) {
            const u64 v = merge_word(words[(size_t)(r * M + j)]);
            for (int b = 0; b < 64; ++b) o[64 * j + b] = (u8)((v >> b) & 1u);
        }
    }
    return out;
}

CellSource SoupBatch::soup_source(const u64* store, i64 first, i64 count) const {
    const i64 S = cfg_.size, M = m(), wps = words_per_soup();
    CellSource s;
    s.base = store + first * wps;
    s.words = count * wps;
    s.frame_stride = wps, s.row_stride = M;
    s.n = count, s.rows = S, s.cols = S;
    s.r0 = 0, s.H = S, s.c0 = 0, s.W = S;
    s.w0 = 0, s.gwords = M, s.fw = M;
    return s;
}

CellTarget SoupBatch::soup_target(u64* store) const {
    CellTarget t;
    t.base = store;
    t.words = cfg_.n * words_per_soup();
    t.row_stride = m(), t.rows = cfg_.n * cfg_.size, t.cols = cfg_.size;
    return t;
}

void SoupBatch::read_boards_cells(i64 first, i64 count, const CellBuffer& dst) {
    if (first < 0 || count < 1 || first > cfg_.n - count)
        throw Error(strprintf("soups: read_boards_cells(): soups %lld .. %lld are outside 0 .. %lld", (long long)first,
                              (long long)(first + count - 1), (long long)cfg_.n - 1));
    if (dst.numel != count * cfg_.size * cfg_.size)
        throw Error(strprintf("soups: read_boards_cells(): the buffer holds %lld elements, the cells are %lld", (long long)dst.numel,
                              (long long)(count * cfg_.size * cfg_.size)));
    do_read_cells(first, count, dst);
}

void SoupBatch::init_cells(const CellBuffer& src) {
    if (src.numel != cfg_.n * cfg_.size * cfg_.size)
        throw Error(strprintf("soups: init_cells(): the buffer holds %lld elements, the cells are %lld", (long long)src.numel,
                              (long long)(cfg_.n * cfg_.size * cfg_.size)));
    do_init_cells(src);
    searching_ = false;
    reached_ = launches_ = settled_ = 0;
}

std::vector<u32> SoupBatch::match_counts(const std::vector<std::vector<MatchTemplate>>& templates) {
    for (const auto& oriented : templates) {
        if (oriented.empty()) throw Error("soups: match_counts(): a template without orientations");
        for (const MatchTemplate& t : oriented) t.validate(cfg_.size, cfg_.size);
    }
    const size_t T = templates.size();
    std::vector<u32> out((size_t)cfg_.n * T, 0), col((size_t)cfg_.n);
    for (size_t t = 0; t < T; ++t) {
        std::fill(col.begin(), col.end(), 0u);
        do_match_counts(templates[t], col.data());
        for (i64 i = 0; i < cfg_.n; ++i) out[(size_t)i * T + t] = col[(size_t)i];
    }
    return out;
}

ComponentsResult SoupBatch::components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) {
    cc_check(cfg_.size, cfg_.size, cfg_.n, max_objects, "soups: components()");
    return do_components(nb, max_objects, hashes, want_records);
}

SoupStats SoupBatch::stats() const {
    SoupStats s;
    s.kernel = strprintf("soups@%lld", (long long)cfg_.size) + (cfg_.rule.is_conway() ? "" : ":rule");
    s.backend = cfg_.backend;
    s.rule = cfg_.rule.str();
    s.launches = launches_;
    s.settled = settled_;
    s.reached = reached_;
    s.workgroup = cfg_.workgroup;
    return s;
}

// ---- CPU backend ----------------------------------------------------------------------------------------------

namespace {

// next = x ? S[T - 1] : B[T] over the four planes of T, the 3 x 3 sum including the centre: decoded count by count.
struct Leaves {
    u64 b[10], s[10];
    explicit Leaves(const Rule& r) {
        for (int t = 0; t < 10; ++t) {
            b[t] = (t <= 8 && ((r.birth >> t) & 1u)) ? ~0ull : 0ull;
            s[t] = (t >= 1 && ((r.survive >> (t - 1)) & 1u)) ? ~0ull : 0ull;
        }
    }
};

inline u64 rule_generic(u64 a0, u64 a1, u64 b0, u64 b1, u64 c0, u64 c1, u64 x, const Leaves& f) {
    const u64 t0 = a0 ^ b0 ^ c0, cy = (a0 & b0) | (a0 & c0) | (b0 & c0);
    const u64 u0 = a1 ^ b1 ^ c1, u1 = (a1 & b1) | (a1 & c1) | (b1 & c1);
    const u64 t1 = cy ^ u0, k = cy & u0, t2 = u1 ^ k, t3 = u1 & k;
    u64 next = 0;
    for (int t = 0; t < 10; ++t) {
        const u64 is = (t & 1 ? t0 : ~t0) & (t & 2 ? t1 : ~t1) & (t & 4 ? t2 : ~t2) & (t & 8 ? t3 : ~t3);
        next |= is & ((x & f.s[t]) | (~x & f.b[t]));
    }
    return next;
}

// One generation of a torus of S rows x M words (split storage): dst from src.  s0 / s1: S * M words of scratch.
void step_soup(const u64* src, u64* dst, i64 S, i64 M, bool conway, const Leaves& f, u64* s0, u64* s1) {
    for (i64 r = 0; r < S; ++r)
        for (i64 j = 0; j < M; ++j) {
            const u64* row = src + r * M;
            hsum64(row[(j + M - 1) % M], row[j], row[(j + 1) % M], s0[r * M + j], s1[r * M + j]);
        }
    for (i64 r = 0; r < S; ++r) {
        const i64 up = ((r + S - 1) % S) * M, mid = r * M, dn = ((r + 1) % S) * M;
        for (i64 j = 0; j < M; ++j)
            dst[mid + j] = conway ? rule64(s0[up + j], s1[up + j], s0[mid + j], s1[mid + j], s0[dn + j], s1[dn + j], src[mid + j])
                                  : rule_generic(s0[up + j], s1[up + j], s0[mid + j], s1[mid + j], s0[dn + j], s1[dn + j],
                                                 src[mid + j], f);
    }
}

u32 count_cells(const u64* b, i64 words) {
    u32 n = 0;
    for (i64 i = 0; i < words; ++i) n += (u32)__builtin_popcountll(b[i]);
    return n;
}

class CpuSoups final : public SoupBatch {
   public:
    explicit CpuSoups(const SoupConfig& c)
        : SoupBatch(c), wps_(words_per_soup()), board_((size_t)(c.n * wps_)), state_((size_t)c.n), conway_(c.rule.is_conway()),
          leaves_(c.rule) {}

   protected:
    void do_init_seed(u64 seed) override {
        const i64 S = cfg_.size, M = m();
#pragma omp parallel for schedule(static)
        for (i64 i = 0; i < cfg_.n; ++i) {
            u64* b = board_.data() + (size_t)(i * wps_);
            for (i64 r = 0; r < S; ++r)
                for (i64 j = 0; j < M; ++j) b[r * M + j] = split_word(random_word(seed + (u64)i, r, j, M));
        }
        reset_states();
    }
    void do_upload(const u64* split) override {
        std::memcpy(board_.data(), split, board_.size() * sizeof(u64));
        reset_states();
    }
    void do_plain(u32 gens) override {
        const i64 S = cfg_.size, M = m();
#pragma omp parallel
        {
            std::vector<u64> tmp((size_t)wps_), s0((size_t)wps_), s1((size_t)wps_);
#pragma omp for schedule(static)
            for (i64 i = 0; i < cfg_.n; ++i) {
                u64* b = board_.data() + (size_t)(i * wps_);
                for (u32 k = 0; k < gens; ++k) {
                    step_soup(b, tmp.data(), S, M, conway_, leaves_, s0.data(), s1.data());
                    std::memcpy(b, tmp.data(), (size_t)wps_ * sizeof(u64));
                }
                state_[(size_t)i].g += gens;
                state_[(size_t)i].population = count_cells(b, wps_);
            }
        }
    }
    void do_begin_search() override {
        saved_ = board_;
        init_ = board_;
        for (SoupState& st : state_) {
            st.s = st.g;
            st.w = 1;
        }
    }
    u64 do_settle(u32 gens, u32 max_gens) override {
        const i64 S = cfg_.size, M = m();
        const size_t bytes = (size_t)wps_ * sizeof(u64);
        i64 settled = 0;
#pragma omp parallel reduction(+ : settled)
        {
            std::vector<u64> tmp((size_t)wps_), s0((size_t)wps_), s1((size_t)wps_);
#pragma omp for schedule(dynamic, 4)
            for (i64 i = 0; i < cfg_.n; ++i) {
                SoupState& st = state_[(size_t)i];
                if (st.period == 0 && st.g < max_gens) {
                    u64* b = board_.data() + (size_t)(i * wps_);
                    u64* sv = saved_.data() + (size_t)(i * wps_);
                    const u32 budget = std::min(gens, max_gens - st.g);
                    for (u32 k = 0; k < budget; ++k) {
                        step_soup(b, tmp.data(), S, M, conway_, leaves_, s0.data(), s1.data());
                        std::memcpy(b, tmp.data(), bytes);
                        ++st.g;
                        if (std::memcmp(b, sv, bytes) == 0) {
                            st.period = st.g - st.s;
                            break;
                        }
                        if (st.g - st.s == st.w) {
                            std::memcpy(sv, b, bytes);
                            st.s = st.g;
                            st.w *= 2;
                        }
                    }
                    st.population = count_cells(b, wps_);
                }
                settled += st.period != 0;
            }
        }
        return (u64)settled;
    }
    u64 do_transient(u32 gens) override {
        const i64 S = cfg_.size, M = m();
        const size_t bytes = (size_t)wps_ * sizeof(u64);
        if (tmp_.empty()) tmp_.resize(board_.size());
        i64 left = 0;
#pragma omp parallel reduction(+ : left)
        {
            std::vector<u64> nxt((size_t)wps_), s0((size_t)wps_), s1((size_t)wps_);
#pragma omp for schedule(dynamic, 4)
            for (i64 i = 0; i < cfg_.n; ++i) {
                SoupState& st = state_[(size_t)i];
                if (st.period == 0 || (st.flags & kSoupTransientDone)) continue;
                // the two copies wait in the soup's saved board (the search is over) and in tmp_
                u64* a = saved_.data() + (size_t)(i * wps_);
                u64* b = tmp_.data() + (size_t)(i * wps_);
                if (!(st.flags & kSoupTransientStarted)) {
                    std::memcpy(a, init_.data() + (size_t)(i * wps_), bytes);
                    std::memcpy(b, a, bytes);
                    st.flags |= kSoupTransientStarted;
                    st.tadv = st.tcount = 0;
                }
                for (u32 k = 0; k < gens; ++k) {
                    if (st.tadv < st.period) {
                        step_soup(b, nxt.data(), S, M, conway_, leaves_, s0.data(), s1.data());
                        std::memcpy(b, nxt.data(), bytes);
                        ++st.tadv;
                        continue;
                    }
                    if (std::memcmp(a, b, bytes) == 0) {
                        st.flags |= kSoupTransientDone;
                        break;
                    }
                    step_soup(a, nxt.data(), S, M, conway_, leaves_, s0.data(), s1.data());
                    std::memcpy(a, nxt.data(), bytes);
                    step_soup(b, nxt.data(), S, M, conway_, leaves_, s0.data(), s1.data());
                    std::memcpy(b, nxt.data(), bytes);
                    ++st.tcount;
                }
                left += !(st.flags & kSoupTransientDone);
            }
        }
        return (u64)left;
    }
    void do_fetch_states(SoupState* out) override { std::memcpy(out, state_.data(), state_.size() * sizeof(SoupState)); }
    void do_fetch_board(i64 soup, u64* split) override {
        std::memcpy(split, board_.data() + (size_t)(soup * wps_), (size_t)wps_ * sizeof(u64));
    }
    void do_read_cells(i64 first, i64 count, const CellBuffer& dst) override {
        unpack_cells_host(soup_source(board_.data(), first, count), dst);
    }
    void do_init_cells(const CellBuffer& src) override {
        pack_cells_host(src, soup_target(board_.data()));
        reset_states();
    }
    void do_match_counts(const std::vector<MatchTemplate>& oriented, u32* counts) override {
#pragma omp parallel
        {
            std::vector<u64> nat((size_t)wps_);
#pragma omp for schedule(static)
            for (i64 i = 0; i < cfg_.n; ++i) {
                const u64* b = board_.data() + (size_t)(i * wps_);
                for (i64 k = 0; k < wps_; ++k) nat[(size_t)k] = merge_word(b[k]);
                u64 c = 0;
                for (const MatchTemplate& t : oriented) c += match_host(nat.data(), cfg_.size, cfg_.size, true, t, nullptr);
                counts[i] = (u32)c;
            }
        }
    }
    ComponentsResult do_components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) override {
        std::vector<u64> nat((size_t)(cfg_.n * wps_));
        for (size_t k = 0; k < nat.size(); ++k) nat[k] = merge_word(board_[k]);
        return components_host(nat.data(), cfg_.size, cfg_.size, cfg_.n, true, nb, max_objects, hashes, want_records, nullptr);
    }

   private:
    void reset_states() {
#pragma omp parallel for schedule(static)
        for (i64 i = 0; i < cfg_.n; ++i) {
            state_[(size_t)i] = SoupState();
            state_[(size_t)i].population = count_cells(board_.data() + (size_t)(i * wps_), wps_);
        }
        saved_.clear();
        init_.clear();
        tmp_.clear();
    }

    i64 wps_;
    std::vector<u64> board_, saved_, init_, tmp_;
    std::vector<SoupState> state_;
    bool conway_;
    Leaves leaves_;
};

}  // namespace

std::unique_ptr<SoupBatch> make_cpu_soups(const SoupConfig& c) { return std::make_unique<CpuSoups>(c); }

}  // namespace gol
