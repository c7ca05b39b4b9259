// gol-mi355x: gfx950 kernels behind the tensor readers and writers (engine.hpp, soups.hpp): dense cells <-> packed
// split words (bits.hpp) where both already are, in HBM.  Two families, each instantiated for the four element types of
// gol/cells.hpp; no LDS, no scratch, vector stores only.  None is on the per-generation path.
//
// k_cells_from_words<T> (unpack) is shaped by its output.  The output, numel elements from `out` on, is cut into the
// 16-byte lines of memory it covers; a thread takes one line (grid-stride), so consecutive lanes store consecutive 16
// bytes with one dwordx4 each.  The 16, 8 or 4 cells of a line come from the one source word that holds them, or, where
// the line crosses a word, the x seam, the window's last column or a row's end, from the runs of the words it crosses
// (CellSource, gol/cells.hpp: one description for board, film slots and soup store).  Only the first and the last line
// can be partial (an `out` that is not 16-byte aligned, a byte count that is no multiple of 16): they are stored element
// by element, inside [out, out + numel).  Every element has one writer.
//
// k_words_from_cells<T> (pack): a wave takes a word of a row, lane l loads the row's element 64 cw + l (coalesced, 64
// consecutive elements), the ballot of "element != 0" is the natural word, and lane 0 stores its split form; lanes past
// the row's last cell vote 0, which masks the row's last word.  Four words per wave are in flight at a time.
#include "gol/bits.hpp"
#include "tensor_kernels.hpp"

namespace gol {
namespace hipk {

namespace {

// element types: the stored integer, the bits of 1, and the sign bit a float comparison with 0 ignores
struct TU8 {
    using elem = u8;
    static constexpr u32 one = 1u, sign = 0u;
};
struct TF16 {
    using elem = uint16_t;
    static constexpr u32 one = 0x3C00u, sign = 0x8000u;
};
struct TBF16 {
    using elem = uint16_t;
    static constexpr u32 one = 0x3F80u, sign = 0x8000u;
};
struct TF32 {
    using elem = u32;
    static constexpr u32 one = 0x3F800000u, sign = 0x80000000u;
};

// a / d for 0 <= a < 2^52, 1 <= d, inv = 1.0 / d: the double product is off by one at most
__device__ __forceinline__ i64 div_by(i64 a, i64 d, double inv) {
    i64 q = (i64)((double)a * inv);
    const i64 r = a - q * d;
    if (r < 0) --q;
    if (r >= d) ++q;
    return q;
}

// bits 0..7 -> eight 0/1 bytes (bit k in byte k)
__device__ __forceinline__ u64 bytes8(u32 bits) {
    const u64 r = ((u64)(bits & 0xFFu) * 0x0101010101010101ull) & 0x8040201008040201ull;  // byte k holds bit k alone
    return ((r + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;                      // non-zero byte -> 1
}

// the cells of one full line (bit x = element x) as 16 bytes at p (16-byte aligned)
template <typename T>
__device__ __forceinline__ void store_line(typename T::elem* p, u32 bits) {
    uint4 v;
    if constexpr (sizeof(typename T::elem) == 1) {
        const u64 lo = bytes8(bits), hi = bytes8(bits >> 8);
        v = make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
    } else if constexpr (sizeof(typename T::elem) == 2) {
        auto pair = [](u32 b) { return ((b & 1u) ? T::one : 0u) | ((b & 2u) ? (T::one << 16) : 0u); };
        v = make_uint4(pair(bits), pair(bits >> 2), pair(bits >> 4), pair(bits >> 6));
    } else {
        v = make_uint4((bits & 1u) ? T::one : 0u, (bits & 2u) ? T::one : 0u, (bits & 4u) ? T::one : 0u, (bits & 8u) ? T::one : 0u);
    }
    *reinterpret_cast<uint4*>(p) = v;
}

template <typename T>
__global__ __launch_bounds__(256) void k_cells_from_words(CellSource s, typename T::elem* __restrict__ out, i64 numel) {
    using E = typename T::elem;
    constexpr int PER = 16 / (int)sizeof(E);
    const i64 lead = (i64)(((uintptr_t)out & 15u) / sizeof(E));  // elements of the first line that lie before out
    const i64 lines = (lead + numel + PER - 1) / PER;
    const double inv_cols = 1.0 / (double)s.cols, inv_rows = 1.0 / (double)s.rows;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < lines; q += (i64)gridDim.x * blockDim.x) {
        i64 e0 = q * PER - lead, e1 = e0 + PER;
        const bool full = e0 >= 0 && e1 <= numel;
        e0 = e0 < 0 ? 0 : e0;
        e1 = e1 > numel ? numel : e1;
        const int need = (int)(e1 - e0);
        // element e0 is column j of output row i of frame k
        const i64 rf = div_by(e0, s.cols, inv_cols);
        i64 j = e0 - rf * s.cols;
        i64 k = div_by(rf, s.rows, inv_rows), i = rf - k * s.rows;
        i64 sr = s.r0 + i;
        sr = sr >= s.H ? sr - s.H : sr;
        const u64* row = s.base + k * s.frame_stride + sr * s.row_stride;
        i64 c = s.c0 + j;
        c = c >= s.W ? c - s.W : c;
        u32 bits = 0;
        for (int got = 0; got < need;) {
            // the run of cells one source word gives: to the word's end, the row's last cell, the window's last column
            const int b = (int)(c & 63);
            i64 run = 64 - b;
            run = run < s.W - c ? run : s.W - c;
            run = run < s.cols - j ? run : s.cols - j;
            run = run < need - got ? run : need - got;
            i64 f = (c >> 6) - s.w0;
            f = f < 0 ? f + s.gwords : f;
            const u32 cells = (u32)(merge_word(row[f]) >> b);
            bits |= (cells & ((1u << (int)run) - 1u)) << got;
            got += (int)run;
            j += run;
            c += run;
            c = c >= s.W ? 0 : c;
            if (j == s.cols && got < need) {  // the line goes on in the next output row
                j = 0;
                if (++i == s.rows) i = 0, ++k;
                sr = s.r0 + i;
                sr = sr >= s.H ? sr - s.H : sr;
                row = s.base + k * s.frame_stride + sr * s.row_stride;
                c = s.c0;
            }
        }
        if (full) {
            store_line<T>(out + e0, bits);
        } else {
            for (int x = 0; x < need; ++x) out[e0 + x] = (E)(((bits >> x) & 1u) ? T::one : 0u);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_words_from_cells(const typename T::elem* __restrict__ in, CellTarget t, i64 nw) {
    using E = typename T::elem;
    constexpr int U = 4;
    const int lane = (int)(threadIdx.x & 63u);
    const i64 wave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    const i64 items = t.rows * nw;
    const double inv_nw = 1.0 / (double)nw;
    for (i64 item0 = wave; item0 < items; item0 += U * nwaves) {
        bool alive[U];
        i64 at[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const i64 item = item0 + u * nwaves;
            alive[u] = false;
            at[u] = -1;
            if (item < items) {
                const i64 r = div_by(item, nw, inv_nw), cw = item - r * nw;
                const i64 col = 64 * cw + lane;
                at[u] = r * t.row_stride + cw;
                if (col < t.cols) alive[u] = (E)(in[r * t.cols + col] & (E)~T::sign) != 0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u64 nat = __ballot(alive[u]);
            if (lane == 0 && at[u] >= 0) t.base[at[u]] = split_word(nat);
        }
    }
}

unsigned tensor_grid(i64 threads, i64 cap = 2048) {
    i64 g = ceil_div(threads, 256);
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

template <typename T>
void unpack(const CellSource& s, const CellBuffer& dst, hipStream_t stream) {
    using E = typename T::elem;
    const i64 lines = ceil_div((i64)(((uintptr_t)dst.ptr & 15u) / sizeof(E)) + dst.numel, 16 / (i64)sizeof(E));
    hipLaunchKernelGGL(k_cells_from_words<T>, dim3(tensor_grid(lines)), dim3(256), 0, stream, s, (E*)dst.ptr, dst.numel);
}

template <typename T>
void pack(const CellBuffer& src, const CellTarget& t, hipStream_t stream) {
    using E = typename T::elem;
    const i64 nw = ceil_div(t.cols, 64);
    hipLaunchKernelGGL(k_words_from_cells<T>, dim3(tensor_grid(ceil_div(t.rows * nw, 4) * 64)), dim3(256), 0, stream,
                       (const E*)src.ptr, t, nw);
}

}  // namespace

void launch_cells_from_words(const CellSource& s, const CellBuffer& dst, hipStream_t stream) {
    check_cells(s, dst, "cells_from_words");
    if (s.cells() >= ((i64)1 << 52)) throw Error("cells_from_words: more than 2^52 cells");
    switch (dst.type) {
        case CellType::U8: return unpack<TU8>(s, dst, stream);
        case CellType::F16: return unpack<TF16>(s, dst, stream);
        case CellType::BF16: return unpack<TBF16>(s, dst, stream);
        case CellType::F32: return unpack<TF32>(s, dst, stream);
    }
}

void launch_words_from_cells(const CellBuffer& src, const CellTarget& t, hipStream_t stream) {
    check_cells(t, src, "words_from_cells");
    if (t.cells() >= ((i64)1 << 52)) throw Error("words_from_cells: more than 2^52 cells");
    switch (src.type) {
        case CellType::U8: return pack<TU8>(src, t, stream);
        case CellType::F16: return pack<TF16>(src, t, stream);
        case CellType::BF16: return pack<TBF16>(src, t, stream);
        case CellType::F32: return pack<TF32>(src, t, stream);
    }
}

void require_device_pointer(const void* ptr, size_t bytes, int device, const char* what) {
    if (!ptr || bytes == 0) throw Error(std::string(what) + ": the buffer is empty or a null pointer");
    for (const u8* p : {(const u8*)ptr, (const u8*)ptr + (bytes - 1)}) {
        hipPointerAttribute_t a;
        const hipError_t e = hipPointerGetAttributes(&a, p);
        if (e != hipSuccess) {
            (void)hipGetLastError();  // (a pointer HIP does not know is an error of the caller, not a sticky one)
            throw Error(strprintf("%s: %p is not device memory (%s); the HIP backend takes tensors on cuda:%d", what, ptr,
                                  hipGetErrorString(e), device));
        }
        if (a.type != hipMemoryTypeDevice || a.device != device)
            throw Error(strprintf("%s: %p is %s memory of device %d; the HIP backend takes tensors on cuda:%d", what, ptr,
                                  a.type == hipMemoryTypeDevice ? "device" : "host or managed", a.device, device));
    }
}

}  // namespace hipk
}  // namespace gol
