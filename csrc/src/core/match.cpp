// gol-mi355x: match templates, their orientations and the host matcher (gol/match.hpp).
#include "gol/match.hpp"

#include <algorithm>

#include "gol/bits.hpp"

namespace gol {

MatchTemplate MatchTemplate::from_pattern(const RlePattern& p, i64 margin) {
    if (margin < 0) throw Error(strprintf("match: margin = %lld is negative", (long long)margin));
    if (p.rows < 1 || p.cols < 1) throw Error("match: the pattern has no cells");
    if (margin > kMatchMaxSide || p.rows + 2 * margin > kMatchMaxSide || p.cols + 2 * margin > kMatchMaxSide)
        throw Error(strprintf("match: a %lld x %lld pattern with margin %lld makes a %lld x %lld template, over %d x %d",
                              (long long)p.rows, (long long)p.cols, (long long)margin, (long long)(p.rows + 2 * margin),
                              (long long)(p.cols + 2 * margin), kMatchMaxSide, kMatchMaxSide));
    MatchTemplate t;
    t.th = (i32)(p.rows + 2 * margin), t.tw = (i32)(p.cols + 2 * margin), t.ring = (i32)margin;
    const u32 all = t.tw == 32 ? ~0u : ((1u << t.tw) - 1u);
    for (int i = 0; i < t.th; ++i) t.care[i] = all;
    for (i64 r = 0; r < p.rows; ++r)
        for (i64 c = 0; c < p.cols; ++c)
            if (p.cell(r, c)) t.value[r + margin] |= 1u << (c + margin);
    return t;
}

MatchTemplate MatchTemplate::from_cells(const u8* value, const u8* care, i64 th, i64 tw, i64 ring) {
    if (th < 1 || tw < 1 || th > kMatchMaxSide || tw > kMatchMaxSide)
        throw Error(strprintf("match: a template of %lld x %lld cells is outside 1 x 1 .. %d x %d", (long long)th, (long long)tw,
                              kMatchMaxSide, kMatchMaxSide));
    if (ring < 0 || ring > kMatchMaxSide) throw Error(strprintf("match: ring = %lld is outside 0 .. %d", (long long)ring, kMatchMaxSide));
    MatchTemplate t;
    t.th = (i32)th, t.tw = (i32)tw, t.ring = (i32)ring;
    for (i64 i = 0; i < th; ++i)
        for (i64 j = 0; j < tw; ++j) {
            if (care[i * tw + j]) t.care[i] |= 1u << j;
            if (value[i * tw + j]) t.value[i] |= 1u << j;
        }
    return t;
}

bool MatchTemplate::operator==(const MatchTemplate& o) const {
    if (th != o.th || tw != o.tw || ring != o.ring) return false;
    for (int i = 0; i < th; ++i)
        if (care[i] != o.care[i] || value[i] != o.value[i]) return false;
    return true;
}

MatchTemplate MatchTemplate::oriented(int k) const {
    if (k < 0 || k > 7) throw Error(strprintf("match: orientation %d is outside 0 .. 7", k));
    MatchTemplate cur = *this;
    if (k >= 4) {  // the left-right mirror image
        MatchTemplate m;
        m.th = th, m.tw = tw, m.ring = ring;
        for (int i = 0; i < th; ++i)
            for (int j = 0; j < tw; ++j) {
                if (cell_care(i, tw - 1 - j)) m.care[i] |= 1u << j;
                if (cell_value(i, tw - 1 - j)) m.value[i] |= 1u << j;
            }
        cur = m;
    }
    for (int turn = 0; turn < (k & 3); ++turn) {  // a quarter turn clockwise: new (i, j) = old (th - 1 - j, i)
        MatchTemplate n;
        n.th = cur.tw, n.tw = cur.th, n.ring = cur.ring;
        for (int i = 0; i < n.th; ++i)
            for (int j = 0; j < n.tw; ++j) {
                if (cur.cell_care(cur.th - 1 - j, i)) n.care[i] |= 1u << j;
                if (cur.cell_value(cur.th - 1 - j, i)) n.value[i] |= 1u << j;
            }
        cur = n;
    }
    return cur;
}

std::vector<std::pair<int, MatchTemplate>> MatchTemplate::orientations(bool all) const {
    std::vector<std::pair<int, MatchTemplate>> out;
    for (int k = 0; k < (all ? 8 : 1); ++k) {
        const MatchTemplate t = oriented(k);
        bool seen = false;
        for (const auto& e : out) seen = seen || e.second == t;
        if (!seen) out.emplace_back(k, t);
    }
    return out;
}

void MatchTemplate::validate(i64 H, i64 W) const {
    if (th < 1 || tw < 1 || th > kMatchMaxSide || tw > kMatchMaxSide)
        throw Error(strprintf("match: a template of %d x %d cells is outside 1 x 1 .. %d x %d", th, tw, kMatchMaxSide, kMatchMaxSide));
    if (ring < 0 || 2 * ring >= std::min(th, tw))
        throw Error(strprintf("match: ring = %d needs 0 <= 2 ring < min(th, tw) = %d", ring, std::min(th, tw)));
    const u32 all = tw == 32 ? ~0u : ((1u << tw) - 1u);
    u32 any = 0;
    for (int i = 0; i < th; ++i) {
        if ((care[i] | value[i]) & ~all) throw Error(strprintf("match: template row %d has cells beyond column %d", i, tw - 1));
        if (value[i] & ~care[i]) {
            int j = 0;
            while (!(((value[i] & ~care[i]) >> j) & 1u)) ++j;
            throw Error(strprintf("match: template cell (%d, %d) has value 1 outside care", i, j));
        }
        any |= care[i];
    }
    if (!any) throw Error(strprintf("match: the %d x %d template has no care cell", th, tw));
    if (H > 0 && th > H) throw Error(strprintf("match: the template has %d rows, the board %lld", th, (long long)H));
    if (W > 0 && tw > W) throw Error(strprintf("match: the template has %d columns, the board %lld", tw, (long long)W));
}

namespace {

// 64 cells of a row from column `start` on (any sign): the torus wraps (start + 64 may pass the seam any number of
// times), the bounded board reads dead cells outside [0, w).
u64 row_bits(const u64* row, i64 w, i64 nw, i64 start, bool torus) {
    if (torus) return wrap64(row, w, start);
    auto word = [&](i64 k) -> u64 { return k < 0 || k >= nw ? 0ull : row[k]; };
    const i64 k = start >= 0 ? start >> 6 : -((-start + 63) >> 6);
    const int off = (int)(start - 64 * k);
    return off ? (word(k) >> off) | (word(k + 1) << (64 - off)) : word(k);
}

}  // namespace

u64 match_host(const u64* words, i64 h, i64 w, bool torus, const MatchTemplate& t, u64* out, bool or_into) {
    const i64 nw = ceil_div(w, 64);
    u64 count = 0;
#pragma omp parallel for schedule(static) reduction(+ : count) if (h * nw > 4096)
    for (i64 r = 0; r < h; ++r)
        for (i64 cw = 0; cw < nw; ++cw) {
            u64 acc = word_mask(cw, w);
            for (int i = 0; i < t.th && acc; ++i) {
                if (!t.care[i]) continue;
                i64 br = r - t.ring + i;
                const u64* row = nullptr;
                if (torus)
                    row = words + pmod(br, h) * nw;
                else if (br >= 0 && br < h)
                    row = words + br * nw;
                for (int j = 0; j < t.tw; ++j) {
                    if (!t.cell_care(i, j)) continue;
                    const u64 bits = row ? row_bits(row, w, nw, 64 * cw + j - t.ring, torus) : 0ull;
                    acc &= t.cell_value(i, j) ? bits : ~bits;
                }
            }
            count += (u64)__builtin_popcountll(acc);
            if (out) out[r * nw + cw] = or_into ? (out[r * nw + cw] | acc) : acc;
        }
    return count;
}

void match_positions_host(const u64* bitmap, i64 h, i64 w, i64 max_hits, std::vector<i32>* out) {
    const i64 nw = ceil_div(w, 64);
    i64 n = 0;
    for (i64 r = 0; r < h && n < max_hits; ++r)
        for (i64 cw = 0; cw < nw && n < max_hits; ++cw)
            for (u64 v = bitmap[r * nw + cw]; v && n < max_hits; v &= v - 1, ++n) {
                out->push_back((i32)r);
                out->push_back((i32)(64 * cw + __builtin_ctzll(v)));
            }
}

}  // namespace gol
