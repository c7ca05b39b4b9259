// gol-mi355x: film mode -- the frames of a board window, one per generation run() computes.
//
// A frame is the window's rows x fw board words in the split word format (bits.hpp): fw is the number of distinct
// board words the window's columns touch, word index f of a frame is the board word (w0 + f) mod gwords, frame row i
// the board row (r0 + i) mod H.  A word is stored whole (all the cells of the board it holds), so the frames of the
// ranks of a job hold disjoint bits and add up without carries; unpack() takes the window's cells out of them.
// Both backends write this format: cpu::superstep on the host, step_film (film_kernel.hip) on the device.
#pragma once

#include <algorithm>
#include <cstring>
#include <string>

#include "gol/bits.hpp"
#include "gol/common.hpp"

namespace gol {

// The window as the caller gives it: window()'s coordinates (global; on the torus r0 and c0 wrap).
struct FilmRect {
    bool on = false;
    i64 r0 = 0, c0 = 0, rows = 0, cols = 0;
    bool operator==(const FilmRect& o) const {
        return on == o.on && r0 == o.r0 && c0 == o.c0 && rows == o.rows && cols == o.cols;
    }
};

constexpr i64 kFilmMaxCells = (i64)1 << 22;  // a larger window is refused (window() reads any rectangle)

// "r0,c0,rows,cols" (GOL_FILM) -> the rectangle; throws Error naming `what` on anything else.
inline FilmRect parse_film(const std::string& s, const char* what = "GOL_FILM") {
    long long v[4] = {0, 0, 0, 0};
    char tail = 0;
    if (sscanf(s.c_str(), " %lld , %lld , %lld , %lld %c", &v[0], &v[1], &v[2], &v[3], &tail) != 4)
        throw Error(std::string(what) + " must be r0,c0,rows,cols (got '" + s + "')");
    return FilmRect{true, v[0], v[1], v[2], v[3]};
}

// The frame geometry of a window of `rows x cols` cells at (r0, c0) on an H x W board (1 <= rows <= H, 1 <= cols <= W).
struct FilmGeo {
    i64 r0 = 0, c0 = 0;  // wrapped into the board
    i64 rows = 0, cols = 0;
    i64 H = 0, W = 0, gwords = 0;
    i64 w0 = 0;  // board word of the window's first column
    i64 fw = 0;  // distinct board words the window's columns touch

    FilmGeo() = default;
    FilmGeo(const FilmRect& f, i64 H_, i64 W_) : rows(f.rows), cols(f.cols), H(H_), W(W_) {
        r0 = pmod(f.r0, H);
        c0 = pmod(f.c0, W);
        gwords = ceil_div(W, 64);
        w0 = c0 >> 6;
        const i64 last = c0 + cols - 1;  // unwrapped
        if (last < W)
            fw = (last >> 6) - w0 + 1;
        else  // across the x seam: words w0 .. gwords - 1, then 0 .. the wrapped last column's (all of them at most)
            fw = std::min(gwords, gwords - w0 + ((last - W) >> 6) + 1);
    }
    i64 slot_words() const { return rows * fw; }
    // frame row of board row g / frame word of board word gw; >= rows / >= fw: not in the window
    i64 frame_row(i64 g) const { return pmod(g - r0, H); }
    i64 frame_word(i64 gw) const { return pmod(gw - w0, gwords); }
    // The window's cells of one frame row (fw packed words) as cols 0/1 bytes: word by word, the run of window
    // columns a board word holds (it ends at the word's end, at the board's last column or at the window's).
    void unpack_row(const u64* frow, u8* out) const {
        for (i64 j = 0; j < cols;) {
            const i64 c = (c0 + j) % W;
            const int b = (int)(c & 63);
            const i64 n = std::min(std::min((i64)64 - b, W - c), cols - j);
            const u64 nat = merge_word(frow[frame_word(c >> 6)]);
            u8 cells[64];
            for (int q = 0; q < 8; ++q) {
                // 8 cells to 8 bytes: bit k of the byte alone in byte k, then any set bit of a byte to its bit 0
                const u64 x = (((nat >> (8 * q)) & 0xFFull) * 0x0101010101010101ull) & 0x8040201008040201ull;
                const u64 y = ((x + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
                for (int k = 0; k < 8; ++k) cells[8 * q + k] = (u8)(y >> (8 * k));  // (one 8-byte store on a little-endian host)
            }
            std::memcpy(out + j, cells + b, (size_t)n);
            j += n;
        }
    }
    // the window's cells of one packed frame as rows x cols 0/1 bytes
    void unpack(const u64* frame, u8* out) const {
        for (i64 i = 0; i < rows; ++i) unpack_row(frame + i * fw, out + i * cols);
    }
};

}  // namespace gol
