// gol-mi355x: gfx950 kernels behind components(), count_components(), components_tensor() and SoupBatch::components()
// (gol/components.hpp): connected-component labelling of the packed board where it is, in HBM and in the split word
// format (bits.hpp).
//
// One thread per board word, lane = word column, as k_match; the geometry is a MatchGeo, so the engine's board and a soup
// batch's store run the same kernels.  A thread un-splits its word (merge_word) and masks it to the row's cells.  The
// nodes of the union-find are the word's runs of ones: a run's head is its lowest cell (x & ~(x << 1); a run that goes on
// from the previous word starts a node of its own at bit 0 and is joined to its left part like any other neighbour), and
// a node's id is its head cell's index b * H * W + r * W + c in the i32 parent array.  Only head slots are ever read or
// written, so the array is never cleared.
//
//   k_cc_init     parent[head] = head.
//   k_cc_merge    per run: the run dilated by the neighbourhood's horizontal reach, ANDed with the three words above it
//                 (moore2: of the two rows above), and the cells to its left in its own row (moore2: across a gap of one
//                 dead cell); one union per distinct overlapping run.  union(a, b): find both roots, then
//                 atomicMin(&parent[hi], lo), and go on from the returned value while it is not hi.
//   k_cc_flatten  every head points at its root.
//   k_cc_roots    the roots (parent[x] == x) are counted with one atomic per wave, which also hands every root a dense id;
//                 the root's slot then holds -(id + 1), and the ids below `cap` get an empty record.
//   k_cc_stats    per run: population and the minima and maxima of the two frames into the root's record.  A thread
//                 combines its runs of one object first, and a wave whose lanes all hold the same object reduces across
//                 the wave before one lane adds.
//   k_cc_hash     per run: the eight orientation sums of its cells inside the finished box (cc_hash_add's keys, the column
//                 keys summed over the run first).
//   k_cc_labels   64 labels per thread, 16-byte stores where the row length allows them.
//
// Termination.  parent[i] <= i holds from k_cc_init on: the only writes are atomicMin.  So a find strictly descends and
// ends at a slot that points at itself, and every retry of a union works on a pair whose larger index is lower than
// before.  No thread waits for another thread's progress: a stale parent (the loads are relaxed agent-scope atomic loads;
// the XCDs' L2s are not coherent for plain loads) is still an ancestor and costs steps only.  The host launches each
// kernel once; nothing iterates until convergence.
//
// Like k_match the kernels read words 0 .. nw - 1 of rows 0 .. h - 1 only: torus neighbours come by wrapped addressing,
// and where w % 64 != 0 the lanes at the column seam build the neighbouring words with wrap64 from the row's own cells and
// map a neighbour cell back to its real word before they look for its run's head.  No LDS.
#include <algorithm>
#include <climits>
#include <vector>

#include "gol/bits.hpp"
#include "gol/components.hpp"
#include "gol/hip_kernels.hpp"

namespace gol {
namespace hipk {

namespace {

__device__ __forceinline__ i32 ld_parent(const i32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[i] <= i always, so x strictly descends and the walk ends at the slot that points at itself.  The path is halved
// with atomicMin on the way (a grandparent is an ancestor below the parent, so the invariant stays).
__device__ __forceinline__ i32 cc_find(i32* parent, i32 x) {
    i32 p = ld_parent(&parent[x]);
    while (p != x) {
        const i32 gp = ld_parent(&parent[p]);
        if (gp != p) atomicMin(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

// Every retry goes on with the pair (old, lo), both below hi: the larger index of the pair strictly falls, so the loop
// ends.  After atomicMin the slot holds min(old, lo); if old was not hi, the link hi -> old was replaced or kept, and
// old and lo still have to be joined.
__device__ __forceinline__ void cc_union(i32* parent, i32 a, i32 b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        const i32 hi = a > b ? a : b, lo = a > b ? b : a;
        const i32 old = atomicMin(&parent[hi], lo);
        if (old == hi) return;
        a = old, b = lo;
    }
}

__device__ __forceinline__ u64 bit_range(int a, int b) { return (~0ull >> (63 - b)) & (~0ull << a); }  // 0 <= a <= b <= 63

struct Word {
    i64 b, r, cw;
    bool valid;
};
// word e of the n = batch * h * nw words (e, n < 2^31); an idle lane shadows word 0
__device__ __forceinline__ Word locate(const MatchGeo& g, i64 e, i64 n) {
    Word x;
    x.valid = e < n;
    const u32 ee = x.valid ? (u32)e : 0u, per = (u32)g.h * (u32)g.nw;
    const u32 b = ee / per, rest = ee - b * per, r = rest / (u32)g.nw;
    x.b = b, x.r = r, x.cw = rest - r * (u32)g.nw;
    return x;
}
__device__ __forceinline__ const u64* board_of(const u64* board, const MatchGeo& g, i64 b) { return board + g.base + b * g.batch_stride; }
// the thread's own word: natural order, cells at columns >= w clear
__device__ __forceinline__ u64 own_word(const u64* brd, const MatchGeo& g, const Word& x) {
    return x.valid ? merge_word(brd[x.r * g.pitch + x.cw]) & word_mask(x.cw, g.w) : 0ull;
}
__device__ __forceinline__ bool seam_lane(const MatchGeo& g, i64 cw) { return g.torus && (g.w & 63) && (cw == 0 || cw >= g.nw - 2); }

// Natural word k (cw - 1 .. cw + 1, so -1 .. nw) of a row as a thread at the seam or elsewhere sees it.
__device__ __forceinline__ u64 seen_word(const MatchGeo& g, const u64* row, i64 k, bool seam) {
    if (seam) return wrap64(SplitRow{row}, g.w, 64 * k);
    if (k < 0 || k >= g.nw) {
        if (!g.torus) return 0ull;
        k = k < 0 ? k + g.nw : k - g.nw;
    }
    return merge_word(row[k]) & word_mask(k, g.w);
}

// The node of the run that holds live bit p of seen word k (value y) of the row whose cell 0 has index rowbase.
__device__ __forceinline__ i32 node_of(const MatchGeo& g, const u64* row, i32 rowbase, i64 k, int p, u64 y, bool seam) {
    if (seam) {  // back to the real word: the seen one may start in the middle of a run or hold the seam
        i64 col = (64 * k + p) % g.w;
        if (col < 0) col += g.w;
        k = col >> 6, p = (int)(col & 63);
        y = merge_word(row[k]) & word_mask(k, g.w);
    } else if (k < 0) {
        k += g.nw;
    } else if (k >= g.nw) {
        k -= g.nw;
    }
    const u64 dead_below = ~y & ((1ull << p) - 1ull);
    const int head = dead_below ? 64 - __clzll((long long)dead_below) : 0;
    return rowbase + (i32)(64 * k + head);
}

// f(p) for one live bit p of every run of y that overlaps mask (each pass clears at least bit p from m)
template <typename F>
__device__ __forceinline__ void for_runs(u64 y, u64 mask, F f) {
    u64 m = y & mask;
    while (m) {
        const int p = __builtin_ctzll(m);
        f(p);
        const u64 t = ~y >> p;
        const int len = t ? __builtin_ctzll(t) : 64 - p;
        m &= ~(len >= 64 ? ~0ull : (((1ull << len) - 1ull) << p));
    }
}

// a := a joined with every run of the row's seen words k - 1, k, k + 1 (values P, C, N) that has a cell in columns
// 64 k + lo .. 64 k + hi (-2 <= lo <= 63, 0 <= hi <= 65, lo <= hi)
__device__ __forceinline__ void link_row(i32* parent, i32 a, const MatchGeo& g, const u64* row, i32 rowbase, i64 k, u64 P,
                                         u64 C, u64 N, int lo, int hi, bool seam) {
    if (lo < 0) for_runs(P, ~0ull << (64 + lo), [&](int p) { cc_union(parent, a, node_of(g, row, rowbase, k - 1, p, P, seam)); });
    if (hi >= 0 && lo <= 63)
        for_runs(C, bit_range(lo < 0 ? 0 : lo, hi > 63 ? 63 : hi), [&](int p) { cc_union(parent, a, node_of(g, row, rowbase, k, p, C, seam)); });
    if (hi > 63) for_runs(N, (1ull << (hi - 63)) - 1ull, [&](int p) { cc_union(parent, a, node_of(g, row, rowbase, k + 1, p, N, seam)); });
}

// f(lo, hi) for every run of ones lo .. hi of x
template <typename F>
__device__ __forceinline__ void for_own_runs(u64 x, F f) {
    while (x) {
        const int lo = __builtin_ctzll(x);
        const u64 t = ~x >> lo;
        const int len = t ? __builtin_ctzll(t) : 64 - lo;
        f(lo, lo + len - 1);
        x &= ~(len >= 64 ? ~0ull : (((1ull << len) - 1ull) << lo));
    }
}

__global__ __launch_bounds__(256) void k_cc_init(const u64* __restrict__ board, MatchGeo g, i32* __restrict__ parent) {
    const i64 n = (i64)g.batch * g.h * g.nw;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const Word x = locate(g, e, n);
        const u64 v = own_word(board_of(board, g, x.b), g, x);
        const i32 base = (i32)((x.b * g.h + x.r) * g.w + 64 * x.cw);
        for (u64 heads = v & ~(v << 1); heads; heads &= heads - 1ull) {
            const i32 id = base + __builtin_ctzll(heads);
            parent[id] = id;
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_merge(const u64* __restrict__ board, MatchGeo g, int nb, i32* parent) {
    const i64 n = (i64)g.batch * g.h * g.nw;
    const int reach = nb == 0 ? 0 : nb;  // columns to either side in a row above: 0, 1, 2
    const int up = nb == 2 ? 2 : 1;      // rows above
    const int gap = nb == 2 ? 1 : 0;     // dead cells two joined cells of a row may have between them
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const Word x = locate(g, e, n);
        const u64* brd = board_of(board, g, x.b);
        const u64 v = own_word(brd, g, x);
        if (!v) continue;
        const bool seam = seam_lane(g, x.cw);
        const i32 board_base = (i32)(x.b * g.h * g.w), rowbase = board_base + (i32)(x.r * g.w);
        const u64* row = brd + x.r * g.pitch;
        // its own row, to the left of a run: the cells lo - 1 - gap .. lo - 1 (the previous word's only for a run at bit 0,
        // or, with a gap, at bit 1)
        const bool look_left = (v & 1ull) || (gap && (v & 2ull));
        const u64 left = look_left ? seen_word(g, row, x.cw - 1, seam) : 0ull;
        for_own_runs(v, [&](int lo, int) {
            link_row(parent, rowbase + (i32)(64 * x.cw + lo), g, row, rowbase, x.cw, left, v, 0ull, lo - 1 - gap, lo - 1, seam);
        });
        for (int d = 1; d <= up; ++d) {
            i64 ra = x.r - d;
            if (ra < 0) {
                if (!g.torus) break;
                ra = (ra % g.h + g.h) % g.h;
            }
            const u64* rowa = brd + ra * g.pitch;
            const u64 P = seen_word(g, rowa, x.cw - 1, seam), C = seen_word(g, rowa, x.cw, seam), N = seen_word(g, rowa, x.cw + 1, seam);
            if (!(P | C | N)) continue;
            const i32 basea = board_base + (i32)(ra * g.w);
            for_own_runs(v, [&](int lo, int hi) {
                link_row(parent, rowbase + (i32)(64 * x.cw + lo), g, rowa, basea, x.cw, P, C, N, lo - reach, hi + reach, seam);
            });
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_flatten(const u64* __restrict__ board, MatchGeo g, i32* parent) {
    const i64 n = (i64)g.batch * g.h * g.nw;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const Word x = locate(g, e, n);
        const u64 v = own_word(board_of(board, g, x.b), g, x);
        const i32 base = (i32)((x.b * g.h + x.r) * g.w + 64 * x.cw);
        for (u64 heads = v & ~(v << 1); heads; heads &= heads - 1ull) {
            const i32 id = base + __builtin_ctzll(heads);
            atomicMin(&parent[id], cc_find(parent, id));
        }
    }
}

// count[0] += the roots; per_board[b] += board b's (nullptr: not kept).  With rec, root number i (in the order of the
// wave's atomic) leaves -(i + 1) in its slot and, for i < cap, an empty record (and zeroed sums).
__global__ __launch_bounds__(256) void k_cc_roots(const u64* __restrict__ board, MatchGeo g, i32* __restrict__ parent,
                                                  u32* __restrict__ count, u32* __restrict__ per_board, CcRecord* __restrict__ rec,
                                                  u64* __restrict__ sums, i64 cap) {
    const int lane = (int)(threadIdx.x & 63u);
    const i64 n = (i64)g.batch * g.h * g.nw, stride = (i64)gridDim.x * blockDim.x;
    i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (i64 e0 = e - lane; e0 < n; e0 += stride, e += stride) {  // (e0: wave-uniform)
        const Word x = locate(g, e, n);
        const u64 v = own_word(board_of(board, g, x.b), g, x);
        const i32 base = (i32)((x.b * g.h + x.r) * g.w + 64 * x.cw);
        u64 roots = 0;
        for (u64 heads = v & ~(v << 1); heads; heads &= heads - 1ull) {
            const int bit = __builtin_ctzll(heads);
            if (parent[base + bit] == base + bit) roots |= 1ull << bit;
        }
        const u32 mine = (u32)__popcll(roots);
        u32 incl = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const u32 t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        const u32 total = __shfl(incl, 63, 64);
        if (total == 0) continue;  // (wave-uniform)
        u32 first = 0;
        if (lane == 63) first = atomicAdd(count, total);
        first = __shfl(first, 63, 64) + incl - mine;
        if (per_board) {  // one atomic where the whole wave lies in one board (lane 0's)
            const i64 b0 = __shfl(x.b, 0, 64);
            if (__all(!x.valid || x.b == b0)) {
                if (lane == 63) atomicAdd(&per_board[b0], total);
            } else if (mine) {
                atomicAdd(&per_board[x.b], mine);
            }
        }
        if (!rec) continue;
        for (; roots; roots &= roots - 1ull, ++first) {
            const i32 id = base + __builtin_ctzll(roots);
            parent[id] = -(i32)first - 1;
            if ((i64)first >= cap) continue;
            CcRecord q;
            q.root = id, q.pop = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) q.ext[k] = (k & 1) ? -1 : INT_MAX;
            rec[first] = q;
            if (sums)
                for (int k = 0; k < 8; ++k) sums[8 * (i64)first + k] = 0ull;
        }
    }
}

// the dense id of the root of the run whose head has index `head` (after k_cc_roots)
__device__ __forceinline__ i64 run_id(const i32* __restrict__ parent, i32 head) {
    i32 p = parent[head];
    if (p >= 0) p = parent[p];
    return -(i64)p - 1;
}

struct Stat {
    i64 id;  // -1: empty
    u32 pop;
    i32 ext[8];
    __device__ __forceinline__ void start(i64 i) {
        id = i, pop = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) ext[k] = (k & 1) ? -1 : INT_MAX;
    }
    // a run of n cells in row r (r2 in the shifted frame) over the columns c0 .. c1 (s0 .. s1 in the shifted frame)
    __device__ __forceinline__ void add(u32 n, i32 r, i32 r2, i32 c0, i32 c1, i32 s0, i32 s1) {
        pop += n;
        ext[0] = min(ext[0], r), ext[1] = max(ext[1], r);
        ext[2] = min(ext[2], c0), ext[3] = max(ext[3], c1);
        ext[4] = min(ext[4], r2), ext[5] = max(ext[5], r2);
        ext[6] = min(ext[6], s0), ext[7] = max(ext[7], s1);
    }
    __device__ __forceinline__ void flush(CcRecord* rec) const {
        if (id < 0) return;
        CcRecord* q = rec + id;
        atomicAdd(&q->pop, pop);
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            atomicMin(&q->ext[k], ext[k]);
            atomicMax(&q->ext[k + 1], ext[k + 1]);
        }
    }
};

__global__ __launch_bounds__(256) void k_cc_stats(const u64* __restrict__ board, MatchGeo g, const i32* __restrict__ parent,
                                                  CcRecord* __restrict__ rec, i64 cap, int wave_reduce) {
    const int lane = (int)(threadIdx.x & 63u);
    const i64 n = (i64)g.batch * g.h * g.nw, stride = (i64)gridDim.x * blockDim.x;
    const i32 H = g.h, W = (i32)g.w;
    i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (i64 e0 = e - lane; e0 < n; e0 += stride, e += stride) {  // (e0: wave-uniform)
        const Word x = locate(g, e, n);
        const u64 v = own_word(board_of(board, g, x.b), g, x);
        const i32 base = (i32)((x.b * g.h + x.r) * g.w + 64 * x.cw);
        const i32 r = (i32)x.r, r2 = (r + H / 2) % H;
        // the thread's first object waits for the wave; a later one is flushed when the next one begins
        Stat head, cur;
        head.start(-1), cur.start(-1);
        for_own_runs(v, [&](int lo, int hi) {
            const i64 id = run_id(parent, base + lo);
            if (id >= cap) return;
            const i32 c0 = (i32)(64 * x.cw) + lo, c1 = (i32)(64 * x.cw) + hi;
            i32 s0 = (c0 + W / 2) % W, s1 = (c1 + W / 2) % W;
            if (s0 > s1) s0 = 0, s1 = W - 1;  // the run holds the shifted frame's seam
            if (head.id < 0) head.start(id);
            if (id == head.id) {
                head.add((u32)(hi - lo + 1), r, r2, c0, c1, s0, s1);
            } else {
                if (id != cur.id) {
                    cur.flush(rec);
                    cur.start(id);
                }
                cur.add((u32)(hi - lo + 1), r, r2, c0, c1, s0, s1);
            }
        });
        cur.flush(rec);
        // one object under all the wave's words (the giant component of a dense board): reduce, then one lane's atomics
        const u64 have = __ballot(head.id >= 0);
        if (have == 0ull) continue;  // (wave-uniform)
        const i64 lead = __shfl(head.id, __builtin_ctzll(have), 64);
        if (wave_reduce && __popcll(have) > 1 && __all(head.id < 0 || head.id == lead)) {
            for (int off = 32; off > 0; off >>= 1) {
                head.pop += __shfl_xor(head.pop, off, 64);
#pragma unroll
                for (int k = 0; k < 8; k += 2) {
                    head.ext[k] = min(head.ext[k], __shfl_xor(head.ext[k], off, 64));
                    head.ext[k + 1] = max(head.ext[k + 1], __shfl_xor(head.ext[k + 1], off, 64));
                }
            }
            head.id = lead;
            if (lane == 0) head.flush(rec);
        } else {
            head.flush(rec);
        }
    }
}

struct Sums {
    i64 id;  // -1: empty
    u64 h[8];
    __device__ __forceinline__ void start(i64 i) {
        id = i;
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = 0ull;
    }
    // a run in box row i: ra, ra2, ga, ga2 the keys of i and rows - 1 - i, the others the column keys summed over the run
    __device__ __forceinline__ void add(u64 ra, u64 ra2, u64 ga, u64 ga2, u64 srb, u64 srb2, u64 sgb, u64 sgb2) {
        h[0] += ra * sgb, h[1] += srb * ga2, h[2] += ra2 * sgb2, h[3] += srb2 * ga;
        h[4] += ra * sgb2, h[5] += srb2 * ga2, h[6] += ra2 * sgb, h[7] += srb * ga;
    }
    __device__ __forceinline__ void flush(u64* sums) const {
        if (id < 0) return;
#pragma unroll
        for (int k = 0; k < 8; ++k) atomicAdd(reinterpret_cast<unsigned long long*>(sums + 8 * id + k), (unsigned long long)h[k]);
    }
};

__global__ __launch_bounds__(256) void k_cc_hash(const u64* __restrict__ board, MatchGeo g, const i32* __restrict__ parent,
                                                 const CcRecord* __restrict__ rec, u64* __restrict__ sums, i64 cap, int wave_reduce) {
    const int lane = (int)(threadIdx.x & 63u);
    const i64 n = (i64)g.batch * g.h * g.nw, stride = (i64)gridDim.x * blockDim.x;
    i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (i64 e0 = e - lane; e0 < n; e0 += stride, e += stride) {  // (e0: wave-uniform)
        const Word x = locate(g, e, n);
        const u64 v = own_word(board_of(board, g, x.b), g, x);
        const i32 base = (i32)((x.b * g.h + x.r) * g.w + 64 * x.cw);
        Sums head, cur;
        head.start(-1), cur.start(-1);
        i64 box_id = -1, r0 = 0, rows = 0, c0 = 0, cols = 0;
        for_own_runs(v, [&](int lo, int hi) {
            const i64 id = run_id(parent, base + lo);
            if (id >= cap) return;
            if (id != box_id) {  // (the boxes are final: k_cc_stats has ended)
                const CcRecord* q = rec + id;
                cc_box_axis(q->ext[0], q->ext[1], q->ext[4], q->ext[5], g.h, g.torus != 0, r0, rows);
                cc_box_axis(q->ext[2], q->ext[3], q->ext[6], q->ext[7], g.w, g.torus != 0, c0, cols);
                box_id = id;
            }
            i64 i = x.r - r0, j = 64 * x.cw + lo - c0;
            if (i < 0) i += g.h;
            if (j < 0) j += g.w;
            const u64 ra = sig_rho((u32)i), ra2 = sig_rho((u32)(rows - 1 - i)), ga = sig_gam((u32)i), ga2 = sig_gam((u32)(rows - 1 - i));
            u64 srb = 0, srb2 = 0, sgb = 0, sgb2 = 0;  // the column keys summed over the run
            for (int t = lo; t <= hi; ++t) {
                const u32 b = (u32)j, b2 = (u32)(cols - 1 - j);
                srb += sig_rho(b), srb2 += sig_rho(b2), sgb += sig_gam(b), sgb2 += sig_gam(b2);
                if (++j >= g.w) j -= g.w;
            }
            if (head.id < 0) head.start(id);
            if (id == head.id) {
                head.add(ra, ra2, ga, ga2, srb, srb2, sgb, sgb2);
            } else {
                if (id != cur.id) {
                    cur.flush(sums);
                    cur.start(id);
                }
                cur.add(ra, ra2, ga, ga2, srb, srb2, sgb, sgb2);
            }
        });
        cur.flush(sums);
        const u64 have = __ballot(head.id >= 0);
        if (have == 0ull) continue;  // (wave-uniform)
        const i64 lead = __shfl(head.id, __builtin_ctzll(have), 64);
        if (wave_reduce && __popcll(have) > 1 && __all(head.id < 0 || head.id == lead)) {
            for (int off = 32; off > 0; off >>= 1)
#pragma unroll
                for (int k = 0; k < 8; ++k) head.h[k] += __shfl_xor(head.h[k], off, 64);
            head.id = lead;
            if (lane == 0) head.flush(sums);
        } else {
            head.flush(sums);
        }
    }
}

// Board 0's labels, (h, w) elements of T = i32 or i64 in row-major order: 1 + the root's index for a live cell, else 0.
// vec: rows and the pointer allow 16-byte stores (w a multiple of four, out aligned to 16 bytes).
template <typename T>
__global__ __launch_bounds__(256) void k_cc_labels(const u64* __restrict__ board, MatchGeo g, const i32* __restrict__ parent,
                                                   T* __restrict__ out, int vec) {
    const i64 n = (i64)g.h * g.nw;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const Word x = locate(g, e, n);
        const u64 v = own_word(board_of(board, g, 0), g, x);
        const i32 base = (i32)(x.r * g.w + 64 * x.cw);
        const i64 cells = g.w - 64 * x.cw < 64 ? g.w - 64 * x.cw : 64;  // of this word
        T* o = out + base;
        T label = 0;
        for (int q = 0; q < 64 && q < cells; q += 4) {
            T l4[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int bit = q + t;
                if (!((v >> bit) & 1ull)) {
                    l4[t] = 0;
                    continue;
                }
                if (bit == 0 || !((v >> (bit - 1)) & 1ull)) {  // a head: its slot holds the root (or, a root's, an id)
                    const i32 p = parent[base + bit];
                    label = (T)(1 + (p < 0 ? base + bit : p));
                }
                l4[t] = label;
            }
            if (vec) {  // (cells is then a multiple of four)
                if constexpr (sizeof(T) == 4) {
                    *reinterpret_cast<int4*>(o + q) = make_int4((int)l4[0], (int)l4[1], (int)l4[2], (int)l4[3]);
                } else {
                    *reinterpret_cast<longlong2*>(o + q) = make_longlong2((long long)l4[0], (long long)l4[1]);
                    *reinterpret_cast<longlong2*>(o + q + 2) = make_longlong2((long long)l4[2], (long long)l4[3]);
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (q + t < cells) o[q + t] = l4[t];
            }
        }
    }
}

unsigned cc_grid(i64 n) {
    const i64 g = ceil_div(n, 256);
    return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

i64 cc_words(const MatchGeo& g, const char* what) {
    if (g.h < 1 || g.nw < 1 || g.w < 1 || g.nw != ceil_div(g.w, 64) || g.pitch < g.nw || g.base < 0 || g.batch < 1 ||
        (g.batch > 1 && g.batch_stride < (i64)g.h * g.pitch))
        throw Error(std::string(what) + ": inconsistent board geometry");
    cc_check(g.h, g.w, g.batch, 1, what);
    return (i64)g.batch * g.h * g.nw;
}

}  // namespace

size_t cc_parent_bytes(const MatchGeo& g) { return (size_t)g.batch * (size_t)g.h * (size_t)g.w * sizeof(i32); }

void launch_cc_init(const u64* board, const MatchGeo& g, i32* parent, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent);
}

void launch_cc_merge(const u64* board, const MatchGeo& g, CcNeighbourhood nb, i32* parent, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    hipLaunchKernelGGL(k_cc_merge, dim3(cc_grid(n)), dim3(256), 0, s, board, g, (int)nb, parent);
}

void launch_cc_flatten(const u64* board, const MatchGeo& g, i32* parent, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    hipLaunchKernelGGL(k_cc_flatten, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent);
}

void launch_cc_roots(const u64* board, const MatchGeo& g, i32* parent, u32* count, u32* per_board, CcRecord* rec, u64* sums,
                     i64 cap, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    if (!count || (rec && cap < 1) || (sums && !rec)) throw Error("components: bad record buffers");
    hipLaunchKernelGGL(k_cc_roots, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent, count, per_board, rec, sums, cap);
}

void launch_cc_stats(const u64* board, const MatchGeo& g, const i32* parent, CcRecord* rec, i64 cap, bool wave_reduce, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    if (!rec || cap < 1) throw Error("components: bad record buffers");
    hipLaunchKernelGGL(k_cc_stats, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent, rec, cap, wave_reduce ? 1 : 0);
}

void launch_cc_hash(const u64* board, const MatchGeo& g, const i32* parent, const CcRecord* rec, u64* sums, i64 cap,
                    bool wave_reduce, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    if (!rec || !sums || cap < 1) throw Error("components: bad record buffers");
    hipLaunchKernelGGL(k_cc_hash, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent, rec, sums, cap, wave_reduce ? 1 : 0);
}

void launch_cc_labels(const u64* board, const MatchGeo& g, const i32* parent, void* out, bool int64, hipStream_t s) {
    const i64 n = cc_words(g, "components");
    if (g.batch != 1 || !out) throw Error("components: labels are written for one board");
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    if (int64)
        hipLaunchKernelGGL(k_cc_labels<i64>, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent, static_cast<i64*>(out),
                           aligned && g.w % 4 == 0 ? 1 : 0);
    else
        hipLaunchKernelGGL(k_cc_labels<i32>, dim3(cc_grid(n)), dim3(256), 0, s, board, g, parent, static_cast<i32*>(out),
                           aligned && g.w % 4 == 0 ? 1 : 0);
}

namespace {

#define CC_HIP(x)                                                                                                    \
    do {                                                                                                             \
        hipError_t e_ = (x);                                                                                         \
        if (e_ != hipSuccess) throw Error(strprintf("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__)); \
    } while (0)

bool g_wave_reduce = true;  // cc_set_wave_reduce(): the measurement switch of k_cc_stats and k_cc_hash

// device scratch of one call, freed when the call ends (also on an error)
struct CcScratch {
    std::vector<void*> p;
    ~CcScratch() {
        for (void* q : p) (void)hipFree(q);
    }
    template <typename T>
    T* get(size_t bytes) {
        void* q = nullptr;
        CC_HIP(hipMalloc(&q, bytes ? bytes : 1));
        p.push_back(q);
        return static_cast<T*>(q);
    }
};

}  // namespace

void cc_set_wave_reduce(bool on) { g_wave_reduce = on; }

void run_component_labels(const u64* board, const MatchGeo& g, CcNeighbourhood nb, void* out, bool int64, hipStream_t s) {
    cc_check(g.h, g.w, g.batch, 1, "components");
    CcScratch scratch;
    i32* parent = scratch.get<i32>(cc_parent_bytes(g));
    launch_cc_init(board, g, parent, s);
    launch_cc_merge(board, g, nb, parent, s);
    launch_cc_flatten(board, g, parent, s);
    launch_cc_labels(board, g, parent, out, int64, s);
    CC_HIP(hipGetLastError());
    CC_HIP(hipStreamSynchronize(s));
}

ComponentsResult run_components(const u64* board, const MatchGeo& g, CcNeighbourhood nb, i64 max_objects, bool hashes,
                                bool want_records, hipStream_t s) {
    cc_check(g.h, g.w, g.batch, max_objects, "components");
    const bool wave_reduce = g_wave_reduce;
    CcScratch scratch;
    i32* parent = scratch.get<i32>(cc_parent_bytes(g));
    const size_t ncount = 1 + (size_t)g.batch;  // the total, then one per board
    u32* count = scratch.get<u32>(ncount * sizeof(u32));
    CcRecord* rec = want_records ? scratch.get<CcRecord>((size_t)max_objects * sizeof(CcRecord)) : nullptr;
    u64* sums = want_records && hashes ? scratch.get<u64>((size_t)max_objects * 8 * sizeof(u64)) : nullptr;
    u32* per_board = g.batch > 1 ? count + 1 : nullptr;  // (one board: the total is its count)
    CC_HIP(hipMemsetAsync(count, 0, ncount * sizeof(u32), s));
    launch_cc_init(board, g, parent, s);
    launch_cc_merge(board, g, nb, parent, s);
    if (want_records) {
        launch_cc_flatten(board, g, parent, s);
        launch_cc_roots(board, g, parent, count, per_board, rec, sums, max_objects, s);
        launch_cc_stats(board, g, parent, rec, max_objects, wave_reduce, s);
        if (hashes) launch_cc_hash(board, g, parent, rec, sums, max_objects, wave_reduce, s);
    } else {
        launch_cc_roots(board, g, parent, count, per_board, nullptr, nullptr, 0, s);
    }
    CC_HIP(hipGetLastError());
    std::vector<u32> counts(ncount);
    CC_HIP(hipMemcpyAsync(counts.data(), count, ncount * sizeof(u32), hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));
    const i64 k = want_records ? (i64)std::min<u64>(counts[0], (u64)max_objects) : 0;
    std::vector<CcRecord> recs((size_t)k);
    std::vector<u64> hs(sums ? (size_t)k * 8 : 0);
    if (k) CC_HIP(hipMemcpyAsync(recs.data(), rec, (size_t)k * sizeof(CcRecord), hipMemcpyDeviceToHost, s));
    if (k && sums) CC_HIP(hipMemcpyAsync(hs.data(), sums, (size_t)k * 8 * sizeof(u64), hipMemcpyDeviceToHost, s));
    CC_HIP(hipStreamSynchronize(s));
    ComponentsResult res = cc_finish(recs.data(), sums ? hs.data() : nullptr, k, counts[0], g.h, g.w, g.torus != 0);
    if (!want_records) res.truncated = false;
    if (g.batch == 1) counts[1] = counts[0];
    res.per_board.assign(counts.begin() + 1, counts.end());
    return res;
}

}  // namespace hipk
}  // namespace gol
