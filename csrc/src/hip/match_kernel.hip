// gol-mi355x: gfx950 kernels behind match(), match_tensor() and SoupBatch::match_counts() (gol/match.hpp): template
// matching on the packed board where it is, in HBM and in the split word format (bits.hpp).
//
// k_match: one thread per board word, lane = word column, a wave = 64 adjacent words of a row (coalesced loads).  The
// accumulator starts as all 64 cells of the word and loses, per constrained template cell, the cells whose board cell
// at that offset has the wrong state: one AND or AND-NOT per 32-bit half with the board word shifted by the cell's
// column offset d = j - ring.  In the split format a shift by an even d is a funnel (v_alignbit_b32) by d / 2 inside
// each half across the word and its neighbour; an odd d swaps the halves, with funnels by (d - 1) / 2 and (d + 1) / 2.
// The template is a kernel argument, so its rows are wave-uniform scalars and the loops over its rows and over the
// set care bits of a row are scalar control flow: a row without care bits costs nothing, and a wave whose 64
// accumulators are all empty leaves the row loop.  The board's geometry is an argument too (MatchGeo), so the engine's
// board (ghost rows and words around it) and a soup batch's store (dense tori) run the same kernel.
//
// Like the view kernels it reads words 0 .. nw - 1 of rows 0 .. h - 1 only, never a ghost: torus neighbours come by
// wrapped addressing, and where w % 64 != 0 the lanes at the column seam build their three words with wrap64 (bits.hpp)
// from the row's own cells; on a bounded board rows and words outside it read as zero.  Cells at columns >= w of the
// last word never match.  No LDS; the match count is reduced over the wave and added with one atomic per wave.
#include "gol/bits.hpp"
#include "gol/hip_kernels.hpp"

namespace gol {
namespace hipk {

namespace {

// 32 bits from bit position 32 prev + 32 + e of the sequence prev : cur : next (|e| <= 16)
__device__ __forceinline__ u32 funnel(u32 prev, u32 cur, u32 next, int e) {
    return e >= 0 ? __funnelshift_r(cur, next, (u32)e) : __funnelshift_r(prev, cur, (u32)(32 + e));
}

__global__ __launch_bounds__(256) void k_match(const u64* __restrict__ board, MatchGeo g, MatchTemplate t,
                                               u64* __restrict__ bitmap, int or_into, u32* __restrict__ count32,
                                               unsigned long long* __restrict__ count64) {
    const int lane = (int)(threadIdx.x & 63u);
    const i64 h = g.h, nw = g.nw;
    const i64 per = h * nw, n = per * g.batch;
    const u64 last_mask = storage_mask(nw - 1, g.w);
    const bool seam = g.torus && (g.w & 63);
    const i64 stride = (i64)gridDim.x * blockDim.x;
    // A thread's words are e, e + stride, ...: their (board, row, word) follow by addition from the one division here.
    i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    i64 nb = e / per, nr = (e - nb * per) / nw, ncw = e - nb * per - nr * nw;
    const i64 sb = stride / per, sr = (stride - sb * per) / nw, scw = stride - sb * per - sr * nw;
    for (i64 e0 = e - lane; e0 < n; e0 += stride, e += stride) {  // (e0: wave-uniform)
        const bool valid = e < n;
        const i64 b = valid ? nb : 0, r = valid ? nr : 0, cw = valid ? ncw : 0;  // idle lanes shadow word 0 and add nothing
        ncw += scw;
        if (ncw >= nw) ncw -= nw, ++nr;
        nr += sr;
        if (nr >= h) nr -= h, ++nb;
        nb += sb;
        const u64* brd = board + g.base + b * g.batch_stride;
        u32 accl = ~0u, acch = ~0u;  // the word's even and odd cells
        for (int i = 0; i < t.th; ++i) {
            const u32 care = t.care[i], val = t.value[i];
            if (!care) continue;
            i64 br = r - t.ring + i;  // (th <= h: at most one wrap)
            bool inside = true;
            if (g.torus)
                br = br < 0 ? br + h : (br >= h ? br - h : br);
            else
                inside = br >= 0 && br < h;
            u64 P = 0, C = 0, N = 0;
            if (inside) {
                const u64* row = brd + br * g.pitch;
                if (seam && (cw == 0 || cw >= nw - 2)) {  // the column seam runs through the partial last word
                    const SplitRow src{row};
                    P = split_word(wrap64(src, g.w, 64 * cw - 64));
                    C = split_word(wrap64(src, g.w, 64 * cw));
                    N = split_word(wrap64(src, g.w, 64 * cw + 64));
                } else {
                    C = row[cw];
                    if (cw == nw - 1) C &= last_mask;
                    if (g.torus) {
                        P = row[cw == 0 ? nw - 1 : cw - 1];
                        N = row[cw == nw - 1 ? 0 : cw + 1];
                    } else {
                        if (cw > 0) P = row[cw - 1];
                        if (cw + 1 < nw) N = row[cw + 1] & (cw + 1 == nw - 1 ? last_mask : ~0ull);
                    }
                }
            }
            const u32 Pl = (u32)P, Ph = (u32)(P >> 32), Cl = (u32)C, Ch = (u32)(C >> 32), Nl = (u32)N, Nh = (u32)(N >> 32);
            for (u32 m = care; m; m &= m - 1u) {
                const int j = __builtin_ctz(m), d = j - t.ring;
                u32 lo, hi;  // the board cells at offset d from the word's even and odd cells
                if (d & 1) {
                    lo = funnel(Ph, Ch, Nh, (d - 1) >> 1);
                    hi = funnel(Pl, Cl, Nl, (d + 1) >> 1);
                } else {
                    lo = funnel(Pl, Cl, Nl, d >> 1);
                    hi = funnel(Ph, Ch, Nh, d >> 1);
                }
                if ((val >> j) & 1u) {
                    accl &= lo;
                    acch &= hi;
                } else {
                    accl &= ~lo;
                    acch &= ~hi;
                }
            }
            if (__ballot(valid && (accl | acch) != 0u) == 0ull) break;
        }
        u64 acc = (u64)accl | ((u64)acch << 32);
        if (cw == nw - 1) acc &= last_mask;
        if (!valid) acc = 0;
        if (bitmap && valid) {
            u64* o = bitmap + g.base + b * g.batch_stride + r * g.pitch + cw;
            *o = or_into ? (*o | acc) : acc;
        }
        u32 c = (u32)__popcll(acc);
        if (__all(!valid || b == __shfl(b, 0, 64))) {  // one board under the whole wave: one atomic
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
            if (lane == 0 && c != 0) {
                if (count32) atomicAdd(&count32[b], c);
                if (count64) atomicAdd(count64, (unsigned long long)c);
            }
        } else if (c != 0) {
            if (count32) atomicAdd(&count32[b], c);
            if (count64) atomicAdd(count64, (unsigned long long)c);
        }
    }
}

// One thread per bitmap word of board 0: its set bits as (row, col) pairs behind an atomic cursor, the first `cap`
// entries stored.  The cursor ends as the number of set bits.
__global__ __launch_bounds__(256) void k_match_positions(const u64* __restrict__ bitmap, MatchGeo g, i32* __restrict__ out,
                                                         i64 cap, unsigned long long* __restrict__ cursor) {
    const i64 nw = g.nw, n = (i64)g.h * nw;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const i64 r = e / nw, cw = e - r * nw;
        u64 v = bitmap[g.base + r * g.pitch + cw];
        if (!v) continue;
        i64 at = (i64)atomicAdd(cursor, (unsigned long long)__popcll(v));
        for (; v && at < cap; v &= v - 1ull, ++at) {
            const int bit = __builtin_ctzll(v);
            out[2 * at] = (i32)r;
            out[2 * at + 1] = (i32)(64 * cw + (bit < 32 ? 2 * bit : 2 * (bit - 32) + 1));
        }
    }
}

unsigned match_grid(i64 n) {
    const i64 g = ceil_div(n, 256);
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

void check_geo(const MatchGeo& g, const char* what) {
    if (g.h < 1 || g.nw < 1 || g.w < 1 || g.nw != ceil_div(g.w, 64) || g.pitch < g.nw || g.base < 0 || g.batch < 1 ||
        (g.batch > 1 && g.batch_stride < (i64)g.h * g.pitch))
        throw Error(std::string(what) + ": inconsistent board geometry");
}

}  // namespace

MatchGeo match_geo(const Layout& L, bool torus) {
    MatchGeo g;
    g.base = L.index(0, 0), g.pitch = L.pitch, g.batch_stride = 0;
    g.w = L.w, g.h = (i32)L.h, g.nw = (i32)L.nw;
    g.torus = torus ? 1 : 0, g.batch = 1;
    return g;
}

void launch_match(const u64* board, const MatchGeo& g, const MatchTemplate& t, u64* bitmap, bool or_into, u32* count32,
                  u64* count64, hipStream_t s) {
    check_geo(g, "match");
    t.validate(g.h, g.w);
    if (!count32 && !count64) throw Error("match: no counter");
    if (g.batch > 1 && (count64 || !count32)) throw Error("match: a batch counts into one u32 per board");
    const i64 n = (i64)g.h * g.nw * g.batch;
    hipLaunchKernelGGL(k_match, dim3(match_grid(n)), dim3(256), 0, s, board, g, t, bitmap, or_into ? 1 : 0, count32,
                       reinterpret_cast<unsigned long long*>(count64));
}

void launch_match_positions(const u64* bitmap, const MatchGeo& g, i32* out, i64 cap, u64* cursor, hipStream_t s) {
    check_geo(g, "match positions");
    if (g.batch != 1 || cap < 0 || (cap > 0 && !out) || !cursor) throw Error("match positions: bad arguments");
    hipLaunchKernelGGL(k_match_positions, dim3(match_grid((i64)g.h * g.nw)), dim3(256), 0, s, bitmap, g, out, cap,
                       reinterpret_cast<unsigned long long*>(cursor));
}

}  // namespace hipk
}  // namespace gol
