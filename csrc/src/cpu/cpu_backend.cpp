// gol-mi355x: CPU stepper and host-side board helpers (see cpu.hpp).
#include <algorithm>
#include <cstring>

#include "gol/bits.hpp"
#include "gol/cpu.hpp"
#include "gol/signature.hpp"

namespace gol {
namespace cpu {

namespace {

// Generic life-like rule, still bit-packed: the four planes of T (the 3x3 sum including the centre, 0..9)
// from the three rows' horizontal sums, then next = x ? S[T - 1] : B[T] as two mux trees over T whose
// leaves are all-ones / all-zeros words built once per call from the rule's masks.
struct RuleLeaves {
    u64 b[10], s[10];  // by T: dead-centre and live-centre outcome
    explicit RuleLeaves(const Rule& r) {
        for (int t = 0; t < 10; ++t) {
            b[t] = (t <= 8 && ((r.birth >> t) & 1u)) ? ~0ull : 0ull;        // (T = 9 has a live centre)
            s[t] = (t >= 1 && ((r.survive >> (t - 1)) & 1u)) ? ~0ull : 0ull;  // (T = 0 has a dead centre)
        }
    }
};

inline u64 mux64(u64 sel, u64 one, u64 zero) { return (sel & one) | (~sel & zero); }

inline u64 tree64(const u64* f, u64 t0, u64 t1, u64 t2, u64 t3) {
    const u64 m01 = mux64(t0, f[1], f[0]), m23 = mux64(t0, f[3], f[2]);
    const u64 m45 = mux64(t0, f[5], f[4]), m67 = mux64(t0, f[7], f[6]);
    const u64 lo = mux64(t2, mux64(t1, m67, m45), mux64(t1, m23, m01));
    return mux64(t3, mux64(t0, f[9], f[8]), lo);  // T >= 8: t2 = t1 = 0
}

inline u64 rule64_generic(u64 a0, u64 a1, u64 b0, u64 b1, u64 c0, u64 c1, u64 x, const RuleLeaves& f) {
    const u64 x0 = a0 ^ b0 ^ c0;
    const u64 cy = (a0 & b0) | (a0 & c0) | (b0 & c0);
    const u64 u0 = a1 ^ b1 ^ c1;
    const u64 u1 = (a1 & b1) | (a1 & c1) | (b1 & c1);
    // T = x0 + 2 (cy + u0 + 2 u1)
    const u64 t1 = cy ^ u0, k = cy & u0, t2 = u1 ^ k, t3 = u1 & k;
    return mux64(x, tree64(f.s, x0, t1, t2, t3), tree64(f.b, x0, t1, t2, t3));
}

// The von Neumann and hexagonal neighbourhoods (rule.hpp): the neighbours are whole words here -- the rows above and
// below as they are, and every cell's west / east neighbour gathered into its own bit position -- counted one by one
// into a three-plane counter (0..6), and the rule is decoded count by count:  next = OR over c of
// [count == c] & (x ? S[c] : B[c]).  The count excludes the centre.
// Split format: the west neighbour of an even cell is the odd cell before it (the odd half shifted up, bit 0 from
// the previous word), that of an odd cell the even cell of the same bit; east is the mirror image.
inline u64 west64(u64 prev, u64 cur) {
    const u32 lo = (u32)cur, hi = (u32)(cur >> 32), prevhi = (u32)(prev >> 32);
    return (u64)((hi << 1) | (prevhi >> 31)) | ((u64)lo << 32);
}
inline u64 east64(u64 cur, u64 next) {
    const u32 lo = (u32)cur, hi = (u32)(cur >> 32), nextlo = (u32)next;
    return (u64)hi | ((u64)((lo >> 1) | (nextlo << 31)) << 32);
}

struct Count3 {
    u64 n0 = 0, n1 = 0, n2 = 0;
    void add(u64 v) {
        const u64 c0 = n0 & v, c1 = n1 & c0;
        n0 ^= v;
        n1 ^= c0;
        n2 ^= c1;
    }
    u64 is(int c) const { return (c & 1 ? n0 : ~n0) & (c & 2 ? n1 : ~n1) & (c & 4 ? n2 : ~n2); }
};

void step_rows_nbhd(const u64* src, u64* dst, const Layout& L, i64 r_lo, i64 r_hi, const Rule& rule) {
    const bool hex = rule.nbhd == Nbhd::Hex;
    const int top = nbhd_max_count(rule.nbhd);
    const i64 n = L.nw + 2;  // words -1 .. nw
#pragma omp parallel for schedule(static) if ((r_hi - r_lo) * n > 16384)
    for (i64 r = r_lo; r < r_hi; ++r) {
        const u64* up = src + L.index(r - 1, -1);
        const u64* mid = src + L.index(r, -1);
        const u64* dn = src + L.index(r + 1, -1);
        u64* out = dst + L.index(r, -1);
        for (i64 j = 0; j < n; ++j) {
            Count3 cnt;
            cnt.add(up[j]);                                      // N
            cnt.add(dn[j]);                                      // S
            cnt.add(west64(j ? mid[j - 1] : 0, mid[j]));         // W
            cnt.add(east64(mid[j], j + 1 < n ? mid[j + 1] : 0));  // E
            if (hex) {
                cnt.add(west64(j ? up[j - 1] : 0, up[j]));          // NW
                cnt.add(east64(dn[j], j + 1 < n ? dn[j + 1] : 0));  // SE
            }
            const u64 x = mid[j];
            u64 next = 0;
            for (int c = 0; c <= top; ++c) {
                const u64 born = (rule.birth >> c) & 1u ? ~x : 0, stays = (rule.survive >> c) & 1u ? x : 0;
                next |= cnt.is(c) & (born | stays);
            }
            out[j] = next;
        }
    }
}

void step_rows_generic(const u64* src, u64* dst, const Layout& L, i64 r_lo, i64 r_hi, const Rule& rule) {
    if (rule.nbhd != Nbhd::Moore) return step_rows_nbhd(src, dst, L, r_lo, r_hi, rule);
    const RuleLeaves f(rule);
    const i64 n = L.nw + 2;  // words -1 .. nw
#pragma omp parallel for schedule(static) if ((r_hi - r_lo) * n > 16384)
    for (i64 r = r_lo; r < r_hi; ++r) {
        const u64* up = src + L.index(r - 1, -1);
        const u64* mid = src + L.index(r, -1);
        const u64* dn = src + L.index(r + 1, -1);
        u64* out = dst + L.index(r, -1);
        for (i64 j = 0; j < n; ++j) {
            u64 pu = j ? up[j - 1] : 0, nu = j + 1 < n ? up[j + 1] : 0;
            u64 pm = j ? mid[j - 1] : 0, nm = j + 1 < n ? mid[j + 1] : 0;
            u64 pd = j ? dn[j - 1] : 0, nd = j + 1 < n ? dn[j + 1] : 0;
            u64 a0, a1, b0, b1, c0, c1;
            hsum64(pu, up[j], nu, a0, a1);
            hsum64(pm, mid[j], nm, b0, b1);
            hsum64(pd, dn[j], nd, c0, c1);
            out[j] = rule64_generic(a0, a1, b0, b1, c0, c1, mid[j], f);
        }
    }
}

}  // namespace

void mask_rows(u64* buf, const Layout& L, i64 r_lo, i64 r_hi, const Edges& edges) {
    if (!edges.dead()) return;
    const i64 n = L.nw + 2, gwords = ceil_div(edges.cols, 64);
    const u64 tail = storage_mask(gwords - 1, edges.cols);
    for (i64 r = r_lo; r < r_hi; ++r) {
        u64* row = buf + L.index(r, -1);
        const i64 gr = edges.row0 + r;
        if (gr < 0 || gr >= edges.rows) {
            std::memset(row, 0, (size_t)n * 8);
            continue;
        }
        for (i64 j = 0; j < n; ++j) {
            const i64 gw = edges.word0 + j - 1;
            if (gw < 0 || gw >= gwords)
                row[j] = 0;
            else if (gw == gwords - 1)
                row[j] &= tail;
        }
    }
}

void step_rows(const u64* src, u64* dst, const Layout& L, i64 r_lo, i64 r_hi, const Rule& rule, const Edges& edges) {
    if (edges.dead()) {  // the torus step, then the cells outside the board cleared
        step_rows(src, dst, L, r_lo, r_hi, rule, Edges());
        return mask_rows(dst, L, r_lo, r_hi, edges);
    }
    if (!rule.is_conway()) return step_rows_generic(src, dst, L, r_lo, r_hi, rule);  // (one branch per call)
    const i64 n = L.nw + 2;  // words -1 .. nw
#pragma omp parallel for schedule(static) if ((r_hi - r_lo) * n > 16384)
    for (i64 r = r_lo; r < r_hi; ++r) {
        const u64* up = src + L.index(r - 1, -1);
        const u64* mid = src + L.index(r, -1);
        const u64* dn = src + L.index(r + 1, -1);
        u64* out = dst + L.index(r, -1);
        for (i64 j = 0; j < n; ++j) {
            u64 pu = j ? up[j - 1] : 0, nu = j + 1 < n ? up[j + 1] : 0;
            u64 pm = j ? mid[j - 1] : 0, nm = j + 1 < n ? mid[j + 1] : 0;
            u64 pd = j ? dn[j - 1] : 0, nd = j + 1 < n ? dn[j + 1] : 0;
            u64 a0, a1, b0, b1, c0, c1;
            hsum64(pu, up[j], nu, a0, a1);
            hsum64(pm, mid[j], nm, b0, b1);
            hsum64(pd, dn[j], nd, c0, c1);
            out[j] = rule64(a0, a1, b0, b1, c0, c1, mid[j]);
        }
    }
}

namespace {

// The tile's own words of `buf` that are words of the window, into the packed frame (cpu.hpp FilmOut).
void film_frame(const u64* buf, const Layout& L, const Edges& edges, const FilmGeo& geo, u64* frame) {
    for (i64 r = 0; r < L.h; ++r) {
        const i64 fr = geo.frame_row(edges.row0 + r);
        if (fr >= geo.rows) continue;
        const u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) {
            const i64 f = geo.frame_word(edges.word0 + c);
            if (f < geo.fw) frame[fr * geo.fw + f] |= row[c] & storage_mask(c, L.w);
        }
    }
}

// The live cells of the tile's own words of `buf`, added to the counts of their blocks (cpu.hpp DensityOut).
void density_map(const u64* buf, const Layout& L, const Edges& edges, const DensityGeo& geo, u64* slot) {
    // (the slot is u64 words, two counts each: counted in u32 of their own and copied over, not through a cast pointer)
    std::vector<u32> counts((size_t)(2 * geo.slot_words()));
    memcpy(counts.data(), slot, counts.size() * sizeof(u32));
    for (i64 r = 0; r < L.h; ++r) {
        const u64* row = buf + L.index(r, 0);
        u32* line = counts.data() + ((edges.row0 + r) / geo.block_rows) * geo.grid_cols;
        for (i64 c = 0; c < L.nw; ++c)
            line[(edges.word0 + c) / geo.block_words] += (u32)__builtin_popcountll(row[c] & storage_mask(c, L.w));
    }
    memcpy(slot, counts.data(), counts.size() * sizeof(u32));
}

}  // namespace

void envelope_or(u64* envelope, const u64* board, const Layout& L) {
    for (i64 r = 0; r < L.h; ++r) {
        const u64* row = board + L.index(r, 0);
        u64* erow = envelope + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) erow[c] |= row[c] & storage_mask(c, L.w);
    }
}

namespace {

// One generation of a Generations rule for rows [r_lo, r_hi) (words -1 .. nw): the live plane of dst holds R, the
// two-state step of the source's live plane; A is the source's live plane and d its decay counter (planes 1 .. M).
//   A' = R & ~any(d)                                             a dying cell is not born
//   d' = (A & ~R) ? 1 : (any(d) & d != C - 2 ? d + 1 : 0)          a cell that fails to survive starts to decay
void gen_rows(const u64* src, u64* dst, const Layout& L, i64 plane_stride, i64 r_lo, i64 r_hi, const Rule& rule) {
    const int M = rule.decay_planes();
    const unsigned last = (unsigned)rule.states - 2u;
    const i64 n = L.nw + 2;
#pragma omp parallel for schedule(static) if ((r_hi - r_lo) * n > 16384)
    for (i64 r = r_lo; r < r_hi; ++r) {
        const i64 at = L.index(r, -1);
        for (i64 j = 0; j < n; ++j) {
            const u64 A = src[at + j], R = dst[at + j];
            u64 d[3] = {0, 0, 0}, any = 0, eq = ~0ull;
            for (int m = 0; m < M; ++m) {
                d[m] = src[(m + 1) * plane_stride + at + j];
                any |= d[m];
                eq &= (last >> m) & 1u ? d[m] : ~d[m];
            }
            const u64 start = A & ~R, keep = any & ~eq;
            dst[at + j] = R & ~any;
            u64 carry = ~0ull;  // d + 1: a ripple over the planes
            for (int m = 0; m < M; ++m) {
                const u64 sum = d[m] ^ carry;
                carry &= d[m];
                dst[(m + 1) * plane_stride + at + j] = (keep & sum) | (m == 0 ? start : 0);
            }
        }
    }
}

u64* superstep_generations(u64* a, u64* b, const Layout& L, int k, const Rule& rule, const Edges& edges, i64 plane_stride) {
    if (plane_stride < L.words())
        throw Error(strprintf("superstep: a plane stride of %lld words is less than a board of %lld", (long long)plane_stride,
                              (long long)L.words()));
    Rule two = rule;  // the births and survivals: the life-like rule with the same masks
    two.states = 2;
    const int M = rule.decay_planes();
    u64* src = a;
    u64* dst = b;
    for (int m = 0; m <= M; ++m) mask_rows(src + m * plane_stride, L, -(i64)k, L.h + k, edges);
    for (int g = 0; g < k; ++g) {
        const i64 ext = k - 1 - g;
        step_rows(src, dst, L, -ext, L.h + ext, two, edges);
        gen_rows(src, dst, L, plane_stride, -ext, L.h + ext, rule);
        std::swap(src, dst);
    }
    return src;
}

}  // namespace

void state_counts(const u64* buf, const Layout& L, i64 plane_stride, const Rule& rule, u64* counts) {
    const int M = rule.decay_planes();
    for (i64 r = 0; r < L.h; ++r)
        for (i64 c = 0; c < L.nw; ++c) {
            const i64 at = L.index(r, c);
            const u64 own = storage_mask(c, L.w), A = buf[at] & own;
            u64 any = 0;
            for (int m = 0; m < M; ++m) any |= buf[(m + 1) * plane_stride + at];
            counts[0] += (u64)__builtin_popcountll(own & ~A & ~any);
            counts[1] += (u64)__builtin_popcountll(A);
            for (int s = 2; s < (int)rule.states; ++s) {
                u64 is = own;  // d == s - 1
                for (int m = 0; m < M; ++m) {
                    const u64 p = buf[(m + 1) * plane_stride + at];
                    is &= ((s - 1) >> m) & 1 ? p : ~p;
                }
                counts[s] += (u64)__builtin_popcountll(is);
            }
        }
}

namespace {

// One generation of a Larger than Life rule (rule.hpp) on the tile's own cells, which are the whole board (one rank):
// the cells unpacked into a frame of `range` more cells on every side (the torus: the board repeated; a bounded board:
// zeros), its summed-area table, and per cell the box sum T INCLUDING the centre against the rule's four thresholds.
// Rows [0, h) of dst are written whole (ghost words zero: the caller refreshes them as after any superstep).
void ltl_generation(const u64* src, u64* dst, const Layout& L, const Rule& rule, bool dead) {
    const i64 h = L.h, w = L.w, R = rule.range, fh = h + 2 * R, fw = w + 2 * R;
    const Rule::LtlThresholds t = rule.ltl_thresholds();
    std::vector<u8> cells((size_t)(h * w));
    for (i64 r = 0; r < h; ++r)
        for (i64 c = 0; c < w; ++c) cells[(size_t)(r * w + c)] = (u8)((src[L.index(r, c >> 6)] >> storage_bit(c)) & 1ull);
    // sat[(r + 1) * (fw + 1) + (c + 1)]: the live cells of frame rows [0, r] x frame columns [0, c]
    std::vector<i32> sat((size_t)((fh + 1) * (fw + 1)), 0);
    for (i64 r = 0; r < fh; ++r) {
        const i64 br = r - R;
        i32 run = 0;
        for (i64 c = 0; c < fw; ++c) {
            const i64 bc = c - R;
            const bool inside = br >= 0 && br < h && bc >= 0 && bc < w;
            if (inside || !dead) run += cells[(size_t)(pmod(br, h) * w + pmod(bc, w))];
            sat[(size_t)((r + 1) * (fw + 1) + c + 1)] = sat[(size_t)(r * (fw + 1) + c + 1)] + run;
        }
    }
    const i64 side = 2 * R + 1;
#pragma omp parallel for schedule(static) if (h * w > 65536)
    for (i64 r = 0; r < h; ++r) {
        u64* out = dst + L.index(r, -1);
        std::memset(out, 0, (size_t)(L.nw + 2) * 8);
        for (i64 c = 0; c < w; ++c) {
            // the box around (r, c) is frame rows [r, r + side) x frame columns [c, c + side)
            const i32 T = sat[(size_t)((r + side) * (fw + 1) + c + side)] - sat[(size_t)(r * (fw + 1) + c + side)] -
                          sat[(size_t)((r + side) * (fw + 1) + c)] + sat[(size_t)(r * (fw + 1) + c)];
            const bool alive = cells[(size_t)(r * w + c)] != 0;
            const bool next = alive ? (T >= (i32)t.slo && T <= (i32)t.shi) : (T >= (i32)t.blo && T <= (i32)t.bhi);
            if (next) out[1 + (c >> 6)] |= 1ull << storage_bit(c);
        }
    }
}

}  // namespace

u64* superstep(u64* a, u64* b, const Layout& L, int k, const Rule& rule, const Edges& edges, u64* counts, u64* sigs,
               const FilmOut& film, const DensityOut& density, u64* envelope, i64 plane_stride) {
    if (rule.ltl()) {
        if (counts || sigs || film.frames || density.maps || envelope)
            throw Error("superstep: the per-generation records and the envelope are not built for Larger than Life rules (" + rule.str() + ")");
        if (k < 1) throw Error(strprintf("superstep depth %d below 1", k));
        if (edges.row0 != 0 || edges.word0 != 0 || (edges.dead() && (edges.rows != L.h || edges.cols != L.w)))
            throw Error("superstep: a Larger than Life rule (" + rule.str() + ") steps a tile that is the whole board (one rank)");
        if (L.h < 2 * (i64)rule.range + 1 || L.w < 2 * (i64)rule.range + 1)
            throw Error(strprintf("superstep: rule %s needs a board of at least %d x %d cells, not %lld x %lld", rule.str().c_str(),
                                  2 * rule.range + 1, 2 * rule.range + 1, (long long)L.h, (long long)L.w));
        for (int g = 0; g < k; ++g) {  // one generation at a time
            ltl_generation(a, b, L, rule, edges.dead());
            std::swap(a, b);
        }
        return a;
    }
    if (k < 1 || k > L.R) throw Error(strprintf("superstep depth %d outside 1..%d", k, L.R));
    if (rule.generations()) {
        if (counts || sigs || film.frames || density.maps || envelope)
            throw Error("superstep: the per-generation records and the envelope are not built for Generations rules (" + rule.str() + ")");
        return superstep_generations(a, b, L, k, rule, edges, plane_stride);
    }
    u64* src = a;
    u64* dst = b;
    mask_rows(src, L, -(i64)k, L.h + k, edges);
    for (int g = 0; g < k; ++g) {
        i64 ext = k - 1 - g;
        step_rows(src, dst, L, -ext, L.h + ext, rule, edges);
        if (counts) counts[g] += population(dst, L);  // the tile's own cells: rows [0, h), words [0, nw), no ghosts
        if (sigs) sigs[g] += signature(dst, L, edges.row0, edges.word0);
        if (film.frames) film_frame(dst, L, edges, *film.geo, film.frames + (i64)g * film.geo->slot_words());
        if (density.maps) density_map(dst, L, edges, *density.geo, density.maps + (i64)g * density.geo->slot_words());
        if (envelope) envelope_or(envelope, dst, L);
        std::swap(src, dst);
    }
    return src;
}

void fill_ghost_cols_wrap(u64* buf, const Layout& L, i64 r_lo, i64 r_hi) {
    for (i64 r = r_lo; r < r_hi; ++r) wrap_row_ghosts(buf + L.index(r, 0), L.w, L.nw);
}

void fill_ghost_rows_wrap(u64* buf, const Layout& L) {
    for (i64 g = 1; g <= L.R; ++g) {
        i64 top = -g, bot = L.h - 1 + g;
        std::memcpy(buf + L.index(top, -1), buf + L.index(pmod(top, L.h), -1), (size_t)L.pitch * 8);
        std::memcpy(buf + L.index(bot, -1), buf + L.index(pmod(bot, L.h), -1), (size_t)L.pitch * 8);
    }
}

void init_tile(u64* buf, const Layout& L, const Geometry& g, const PatternSpec& p) {
    std::memset(buf, 0, (size_t)L.bytes());
    const i64 gwords = g.global_words(), gw0 = g.word0();
#pragma omp parallel for schedule(static) if (L.h * L.nw > 65536)
    for (i64 r = 0; r < L.h; ++r) {
        u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) {
            u64 v = 0;
            if (p.fill == Fill::Ones)
                v = ~0ull;
            else if (p.fill == Fill::Random)
                v = random_word(p.seed, g.row0 + r, gw0 + c, gwords);
            row[c] = split_word(v & L.mask(c));
        }
    }
    for (const auto& rc : p.cells) {
        i64 r = rc.first - g.row0, c = rc.second - g.col0;
        if (r < 0 || r >= L.h || c < 0 || c >= L.w) continue;
        buf[L.index(r, c >> 6)] |= 1ull << storage_bit(c);
    }
}

// Board storage is split-format (bits.hpp); dense words are natural order.
void extract_words(const u64* buf, const Layout& L, u64* dense) {
    for (i64 r = 0; r < L.h; ++r) {
        const u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) dense[r * L.nw + c] = merge_word(row[c]) & L.mask(c);
    }
}

void insert_words(u64* buf, const Layout& L, const u64* dense) {
    for (i64 r = 0; r < L.h; ++r) {
        u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) row[c] = split_word(dense[r * L.nw + c] & L.mask(c));
    }
}

u64 population(const u64* buf, const Layout& L) {
    u64 n = 0;
    for (i64 r = 0; r < L.h; ++r) {
        const u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) n += (u64)__builtin_popcountll(row[c] & storage_mask(c, L.w));
    }
    return n;
}

// Defined on natural-order words, so it does not depend on the storage format.
u64 fingerprint(const u64* buf, const Layout& L, i64 grow0, i64 gword0, i64 gwords) {
    u64 s = 0;
    for (i64 r = 0; r < L.h; ++r) {
        const u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c)
            s += fingerprint_word((u64)(grow0 + r) * (u64)gwords + (u64)(gword0 + c), merge_word(row[c]) & L.mask(c));
    }
    return s;
}

u64 signature(const u64* buf, const Layout& L, i64 grow0, i64 gword0) {
    u64 s = 0;
    for (i64 r = 0; r < L.h; ++r) {
        const u64* row = buf + L.index(r, 0);
        for (i64 c = 0; c < L.nw; ++c) s += signature_word(grow0 + r, gword0 + c, row[c] & storage_mask(c, L.w));
    }
    return s;
}

}  // namespace cpu
}  // namespace gol
