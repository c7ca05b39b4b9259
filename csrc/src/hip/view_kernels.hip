// gol-mi355x: gfx950 kernels behind window(), density() and stamp() (engine.hpp): reading and editing the live
// board where it is, in HBM and in the split word format (bits.hpp), so that a window leaves the device as the
// window's bytes, a density map as its counts, and a stamp arrives as the pattern's words.
//
// All three are grid-stride kernels over rectangles in tile coordinates, clipped to the tile by the caller,
// with one writer per output element: they read words 0 .. nw - 1 of rows 0 .. h - 1 only, never a ghost word
// or a ghost row.  None is on the per-generation path.
#include "gol/bits.hpp"
#include "gol/hip_kernels.hpp"

namespace gol {
namespace hipk {

namespace {

// bits 0..7 -> eight 0/1 bytes (bit k in byte k)
__device__ __forceinline__ u64 bytes8(u64 bits) {
    const u64 r = ((bits & 0xFFull) * 0x0101010101010101ull) & 0x8040201008040201ull;  // byte k holds bit k alone
    return ((r + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;                    // non-zero byte -> 1
}

// One thread per source word of the rectangle (64 cells): merge to natural order, mask the tile's last word,
// then the word's cells inside the rectangle as 0/1 bytes into dst (rows x cols, dense): single bytes up to
// the first 8-byte boundary of the destination, then 16-byte (and at most two 8-byte) stores, then the tail.
__global__ __launch_bounds__(256) void k_window_bytes(const u64* __restrict__ buf, i64 pitch, int R, i64 w, ViewRect rc,
                                                      u8* __restrict__ dst) {
    const i64 cw0 = rc.tc >> 6, nwp = ((rc.tc + rc.cols - 1) >> 6) - cw0 + 1;
    const i64 n = rc.rows * nwp;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const i64 r = e / nwp, cw = cw0 + (e - r * nwp);
        u64 v = merge_word(buf[(rc.tr + r + R) * pitch + cw + 1]) & word_mask(cw, w);
        const i64 lo = rc.tc > 64 * cw ? rc.tc : 64 * cw;
        const i64 hi = rc.tc + rc.cols < 64 * cw + 64 ? rc.tc + rc.cols : 64 * cw + 64;
        int left = (int)(hi - lo);
        v >>= (int)(lo & 63);
        u8* o = dst + r * rc.cols + (lo - rc.tc);
        for (; left > 0 && ((uintptr_t)o & 7u); --left, v >>= 1) *o++ = (u8)(v & 1ull);
        if (left >= 8 && ((uintptr_t)o & 15u)) {
            *reinterpret_cast<u64*>(o) = bytes8(v);
            o += 8, v >>= 8, left -= 8;
        }
        for (; left >= 16; o += 16, v >>= 16, left -= 16)
            *reinterpret_cast<ulonglong2*>(o) = make_ulonglong2(bytes8(v), bytes8(v >> 8));
        if (left >= 8) {
            *reinterpret_cast<u64*>(o) = bytes8(v);
            o += 8, v >>= 8, left -= 8;
        }
        for (; left > 0; --left, v >>= 1) *o++ = (u8)(v & 1ull);
    }
}

struct DensityParams {
    i64 pitch, h, nw;
    i64 row0, gword0;          // global row / word of tile row 0 / word 0
    i64 block_rows, block_words, grid_cols;
    u64 last_mask;             // storage mask of word nw - 1
    i32 R, rows_per_item;
};

// A wave takes a run of rows_per_item rows of 64 adjacent word columns, lane = word column, so that a row of
// the run is one contiguous 512-byte load.  Each lane sums __popcll(word & storage mask) down its column: the
// count needs no merge_word, split storage only permutes the bits of a word, which is why blocks are whole
// words wide.  Where the run ends or crosses into the next row of blocks, the lanes of one block (adjacent
// lanes: a block is block_words columns wide) are summed by a segmented wave reduction and the first lane of
// each block adds the sum to the grid: one atomicAdd per wave and block, i.e. one per wave for blocks of 64
// words or more, and 64 adds to 64 different counters for one-word blocks.
__global__ __launch_bounds__(256) void k_density(const u64* __restrict__ buf, DensityParams p, u32* __restrict__ counts) {
    const int lane = (int)(threadIdx.x & 63u);
    const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    const i64 ngroups = (p.nw + 63) >> 6, nruns = (p.h + p.rows_per_item - 1) / p.rows_per_item;
    for (i64 item = wave; item < ngroups * nruns; item += nwaves) {
        const i64 run = item / ngroups, cw = (item - run * ngroups) * 64 + lane;
        const bool valid = cw < p.nw;
        const int bj = valid ? (int)((p.gword0 + cw) / p.block_words) : -1;
        const u64 mask = cw == p.nw - 1 ? p.last_mask : ~0ull;
        const u64* col = buf + (i64)p.R * p.pitch + cw + 1;  // word cw of row r: col[r * pitch]
        const i64 rend = p.h < (run + 1) * p.rows_per_item ? p.h : (run + 1) * p.rows_per_item;
        for (i64 r = run * p.rows_per_item; r < rend;) {
            const i64 bi = (p.row0 + r) / p.block_rows;
            const i64 edge = (bi + 1) * p.block_rows - p.row0;  // first tile row of the next row of blocks
            const i64 stop = edge < rend ? edge : rend;
            u32 acc = 0;
            if (valid)
                for (i64 q = r; q < stop; ++q) acc += (u32)__popcll(col[q * p.pitch] & mask);
            for (int off = 1; off < 64; off <<= 1) {  // lane i: sum of lanes i .. i + 2 off - 1 of its block
                const u32 v = __shfl_down(acc, off, 64);
                const int k = __shfl_down(bj, off, 64);
                if (lane + off < 64 && k == bj) acc += v;
            }
            const int before = __shfl_up(bj, 1, 64);
            if (valid && acc != 0 && (lane == 0 || before != bj)) atomicAdd(&counts[bi * p.grid_cols + bj], acc);
            r = stop;
        }
    }
}

// One thread per board word of the rectangle: the two pattern words that cover it are funnelled by the column
// offset (extract_bits), split, and combined with the word under the mask of the rectangle's columns in it
// (stamp_word, bits.hpp).  pat: natural-order words, pnw per pattern row; the rectangle's first cell is the
// pattern's cell (pr0, pc0).
__global__ __launch_bounds__(256) void k_stamp(u64* __restrict__ buf, i64 pitch, int R, ViewRect rc,
                                               const u64* __restrict__ pat, i64 pnw, i64 pr0, i64 pc0, int mode) {
    const i64 cw0 = rc.tc >> 6, nwp = ((rc.tc + rc.cols - 1) >> 6) - cw0 + 1;
    const i64 n = rc.rows * nwp;
    for (i64 e = (i64)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (i64)gridDim.x * blockDim.x) {
        const i64 r = e / nwp, cw = cw0 + (e - r * nwp);
        u64* word = buf + (rc.tr + r + R) * pitch + cw + 1;
        *word = stamp_word(*word, pat + (pr0 + r) * pnw, pc0, rc.tc, rc.cols, cw, mode);
    }
}

unsigned view_grid(i64 n, i64 cap = 2048) {
    i64 g = ceil_div(n, 256);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

void check_rect(const Layout& L, const ViewRect& rc, const char* what) {
    if (rc.rows < 1 || rc.cols < 1 || rc.tr < 0 || rc.tc < 0 || rc.tr + rc.rows > L.h || rc.tc + rc.cols > L.w)
        throw Error(strprintf("%s: rectangle %lld+%lld x %lld+%lld outside the %lld x %lld tile", what, (long long)rc.tr,
                              (long long)rc.rows, (long long)rc.tc, (long long)rc.cols, (long long)L.h, (long long)L.w));
}

}  // namespace

void launch_window_bytes(const u64* buf, const Layout& L, const ViewRect& rc, u8* dst, hipStream_t s) {
    check_rect(L, rc, "window");
    const i64 nwp = ((rc.tc + rc.cols - 1) >> 6) - (rc.tc >> 6) + 1;
    hipLaunchKernelGGL(k_window_bytes, dim3(view_grid(rc.rows * nwp)), dim3(256), 0, s, buf, L.pitch, L.R, L.w, rc, dst);
}

void launch_density(const u64* buf, const Layout& L, i64 row0, i64 gword0, i64 block_rows, i64 block_words,
                    i64 grid_cols, u32* counts, hipStream_t s) {
    if (block_rows < 1 || block_words < 1 || grid_cols < 1) throw Error("density: bad block shape");
    DensityParams p;
    p.pitch = L.pitch, p.h = L.h, p.nw = L.nw;
    p.row0 = row0, p.gword0 = gword0;
    p.block_rows = block_rows, p.block_words = block_words, p.grid_cols = grid_cols;
    p.last_mask = storage_mask(L.nw - 1, L.w);
    p.R = L.R;
    // runs short enough for ~8192 waves on a big tile (32 rows at 32768^2), at most 64 rows
    const i64 groups = ceil_div(L.nw, 64);
    const i64 rpi = L.h * groups / 8192;
    p.rows_per_item = (i32)(rpi < 4 ? 4 : (rpi > 64 ? 64 : rpi));
    const i64 items = groups * ceil_div(L.h, p.rows_per_item);
    hipLaunchKernelGGL(k_density, dim3(view_grid(items * 64)), dim3(256), 0, s, buf, p, counts);
}

void launch_stamp(u64* buf, const Layout& L, const ViewRect& rc, const u64* pat, i64 pnw, i64 pr0, i64 pc0, int mode,
                  hipStream_t s) {
    check_rect(L, rc, "stamp");
    if (mode < 0 || mode > 3 || pr0 < 0 || pc0 < 0 || pc0 + rc.cols > 64 * pnw) throw Error("stamp: bad pattern offsets");
    const i64 nwp = ((rc.tc + rc.cols - 1) >> 6) - (rc.tc >> 6) + 1;
    hipLaunchKernelGGL(k_stamp, dim3(view_grid(rc.rows * nwp)), dim3(256), 0, s, buf, L.pitch, L.R, rc, pat, pnw, pr0, pc0,
                       mode);
}

}  // namespace hipk
}  // namespace gol
