// gol-mi355x: connected components on the host (gol/components.hpp): a union-find over the live cells of natural-order
// words, the records' finishing (box rule, hash minimum, order) shared with the HIP backends, and the checks.
#include "gol/components.hpp"

#include <algorithm>
#include <cstdint>
#include <numeric>

namespace gol {

CcNeighbourhood cc_neighbourhood(const std::string& name) {
    if (name == "von_neumann") return CcNeighbourhood::VonNeumann;
    if (name == "moore") return CcNeighbourhood::Moore;
    if (name == "moore2") return CcNeighbourhood::Moore2;
    throw Error("components: neighbourhood '" + name + "' is not one of von_neumann, moore, moore2");
}

const char* cc_neighbourhood_name(CcNeighbourhood nb) {
    return nb == CcNeighbourhood::VonNeumann ? "von_neumann" : (nb == CcNeighbourhood::Moore ? "moore" : "moore2");
}

void cc_check(i64 h, i64 w, i64 batch, i64 max_objects, const char* what) {
    if (max_objects < 1) throw Error(strprintf("%s: max_objects = %lld is less than 1", what, (long long)max_objects));
    if (h < 1 || w < 1 || batch < 1) throw Error(strprintf("%s: no cells", what));
    const long double cells = (long double)h * (long double)w * (long double)batch;
    if (cells >= 2147483648.0L)
        throw Error(strprintf("%s: %lld x %lld cells x %lld boards = %.0Lf cells, and labels are 32-bit: fewer than 2^31 = "
                              "2147483648 cells can be labelled", what, (long long)h, (long long)w, (long long)batch, cells));
}

ComponentsResult cc_finish(const CcRecord* rec, const u64* sums, i64 k, u64 count, i64 h, i64 w, bool torus) {
    ComponentsResult res;
    res.count = count;
    res.truncated = count > (u64)k;
    std::vector<i64> order((size_t)k);
    std::iota(order.begin(), order.end(), (i64)0);
    std::sort(order.begin(), order.end(), [&](i64 a, i64 b) { return rec[a].root < rec[b].root; });
    res.board.reserve((size_t)k), res.anchor.reserve((size_t)(2 * k)), res.population.reserve((size_t)k);
    res.bbox.reserve((size_t)(4 * k));
    if (sums) res.hash.reserve((size_t)k);
    const i64 per = h * w;
    for (i64 i : order) {
        const CcRecord& q = rec[i];
        const i64 cell = q.root % per;
        res.board.push_back(q.root / per);
        res.anchor.push_back(cell / w);
        res.anchor.push_back(cell % w);
        res.population.push_back(q.pop);
        i64 r0, rows, c0, cols;
        cc_box_axis(q.ext[0], q.ext[1], q.ext[4], q.ext[5], h, torus, r0, rows);
        cc_box_axis(q.ext[2], q.ext[3], q.ext[6], q.ext[7], w, torus, c0, cols);
        res.bbox.insert(res.bbox.end(), {r0, c0, rows, cols});
        if (sums) res.hash.push_back(*std::min_element(sums + 8 * i, sums + 8 * i + 8));
    }
    return res;
}

u64 object_hash_host(const u8* cells, i64 rows, i64 cols) {
    u64 hk[8] = {};
    for (i64 i = 0; i < rows; ++i)
        for (i64 j = 0; j < cols; ++j)
            if (cells[i * cols + j]) cc_hash_add(hk, i, j, rows, cols);
    return *std::min_element(hk, hk + 8);
}

namespace {

// parent[x] <= x always, so the walk strictly descends and ends at a root; the path is halved on the way
i32 find(std::vector<i32>& parent, i32 x) {
    while (parent[(size_t)x] != x) {
        parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
        x = parent[(size_t)x];
    }
    return x;
}

void unite(std::vector<i32>& parent, i32 a, i32 b) {
    a = find(parent, a), b = find(parent, b);
    if (a < b)
        parent[(size_t)b] = a;
    else if (b < a)
        parent[(size_t)a] = b;
}

}  // namespace

ComponentsResult components_host(const u64* words, i64 h, i64 w, i64 batch, bool torus, CcNeighbourhood nb, i64 max_objects,
                                 bool hashes, bool want_records, i32* labels) {
    cc_check(h, w, batch, max_objects, "components");
    const i64 nw = ceil_div(w, 64), per = h * w;
    // the neighbours that come earlier in row-major order on an unwrapped board (the relation is symmetric, so the
    // other half follows); reach 2 for moore2
    std::vector<std::pair<int, int>> back;
    const int reach = nb == CcNeighbourhood::Moore2 ? 2 : 1;
    for (int dr = -reach; dr <= 0; ++dr)
        for (int dc = -reach; dc <= reach; ++dc) {
            if (dr == 0 && dc >= 0) break;
            if (nb == CcNeighbourhood::VonNeumann && dr != 0 && dc != 0) continue;
            back.emplace_back(dr, dc);
        }
    std::vector<CcRecord> recs;
    std::vector<u64> sums;
    std::vector<u32> per_board((size_t)batch, 0);
    u64 count = 0;
    std::vector<i32> parent((size_t)per), id;
    for (i64 b = 0; b < batch; ++b) {
        const u64* brd = words + b * h * nw;
        auto alive = [&](i64 r, i64 c) { return (brd[r * nw + (c >> 6)] >> (c & 63)) & 1ull; };
        for (i64 r = 0; r < h; ++r)
            for (i64 c = 0; c < w; ++c)
                if (alive(r, c)) parent[(size_t)(r * w + c)] = (i32)(r * w + c);
        for (i64 r = 0; r < h; ++r)
            for (i64 cw = 0; cw < nw; ++cw)
                for (u64 v = brd[r * nw + cw]; v; v &= v - 1) {
                    const i64 c = 64 * cw + __builtin_ctzll(v);
                    for (const auto& d : back) {
                        i64 rr = r + d.first, cc = c + d.second;
                        if (torus)
                            rr = pmod(rr, h), cc = pmod(cc, w);
                        else if (rr < 0 || cc < 0 || cc >= w)
                            continue;
                        if (alive(rr, cc)) unite(parent, (i32)(r * w + c), (i32)(rr * w + cc));
                    }
                }
        // roots in row-major order are the anchors in their final order
        const i64 first = (i64)recs.size();
        if (want_records) id.assign((size_t)per, -1);
        for (i64 r = 0; r < h; ++r)
            for (i64 cw = 0; cw < nw; ++cw)
                for (u64 v = brd[r * nw + cw]; v; v &= v - 1) {
                    const i64 c = 64 * cw + __builtin_ctzll(v);
                    const i32 x = (i32)(r * w + c), root = find(parent, x);
                    parent[(size_t)x] = root;
                    if (labels) labels[b * per + x] = 1 + root;
                    if (root == x) {
                        ++count, ++per_board[(size_t)b];
                        if (want_records && (i64)recs.size() < max_objects) {
                            id[(size_t)x] = (i32)recs.size();
                            recs.push_back(CcRecord{(i32)(b * per + x), 0u, {INT32_MAX, -1, INT32_MAX, -1, INT32_MAX, -1, INT32_MAX, -1}});
                        }
                    }
                    if (!want_records || id[(size_t)root] < 0) continue;
                    CcRecord& q = recs[(size_t)id[(size_t)root]];
                    const i32 v4[4] = {(i32)r, (i32)c, (i32)((r + h / 2) % h), (i32)((c + w / 2) % w)};
                    q.pop += 1;
                    q.ext[0] = std::min(q.ext[0], v4[0]), q.ext[1] = std::max(q.ext[1], v4[0]);
                    q.ext[2] = std::min(q.ext[2], v4[1]), q.ext[3] = std::max(q.ext[3], v4[1]);
                    q.ext[4] = std::min(q.ext[4], v4[2]), q.ext[5] = std::max(q.ext[5], v4[2]);
                    q.ext[6] = std::min(q.ext[6], v4[3]), q.ext[7] = std::max(q.ext[7], v4[3]);
                }
        if (labels)
            for (i64 r = 0; r < h; ++r)
                for (i64 c = 0; c < w; ++c)
                    if (!alive(r, c)) labels[b * per + r * w + c] = 0;
        if (!want_records || !hashes) continue;
        sums.resize(recs.size() * 8, 0);
        for (i64 r = 0; r < h; ++r)
            for (i64 cw = 0; cw < nw; ++cw)
                for (u64 v = brd[r * nw + cw]; v; v &= v - 1) {
                    const i64 c = 64 * cw + __builtin_ctzll(v);
                    const i32 k = id[(size_t)parent[(size_t)(r * w + c)]];  // (every cell points at its root by now)
                    if (k < first) continue;
                    const CcRecord& q = recs[(size_t)k];
                    i64 r0, rows, c0, cols;
                    cc_box_axis(q.ext[0], q.ext[1], q.ext[4], q.ext[5], h, torus, r0, rows);
                    cc_box_axis(q.ext[2], q.ext[3], q.ext[6], q.ext[7], w, torus, c0, cols);
                    cc_hash_add(&sums[(size_t)k * 8], pmod(r - r0, h), pmod(c - c0, w), rows, cols);
                }
    }
    ComponentsResult res = cc_finish(recs.data(), hashes && want_records ? sums.data() : nullptr, (i64)recs.size(), count, h, w, torus);
    if (!want_records) res.truncated = false;
    res.per_board = per_board;
    return res;
}

}  // namespace gol
