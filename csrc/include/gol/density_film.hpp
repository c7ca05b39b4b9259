// gol-mi355x: density-film mode -- the density map of the whole board, one per generation run() computes.
//
// A map is what Engine::density(block_rows, block_cols) returns: grid_rows x grid_cols u32 counts, row-major, the
// live cells of block (bi, bj) of the global board at [bi * grid_cols + bj]; block_cols is a multiple of 64, so a
// board word lies in one block column.  A generation's slot is that grid padded to a whole number of u64 words (two
// counts per word, the first in the low half on the little-endian hosts and devices this runs on).  Every rank adds
// the cells it owns into a zeroed slot, so the slots of the ranks of a job add up count by count; a block holds
// fewer than 2^32 cells, so the sum of two u64 words carries nothing from the low count into the high one.
// Both backends write this format: cpu::superstep on the host, step_density (density_kernel.hip) on the device.
#pragma once

#include <cstdio>
#include <string>

#include "gol/common.hpp"

namespace gol {

// The blocks as the caller gives them: density()'s block shape.
struct DensityBlocks {
    bool on = false;
    i64 rows = 0, cols = 0;
    bool operator==(const DensityBlocks& o) const { return on == o.on && rows == o.rows && cols == o.cols; }
};

constexpr i64 kDensityFilmMaxBlocks = (i64)1 << 20;  // a finer grid is refused (density() takes any)

// "block_rows[,block_cols]" (GOL_DENSITY_FILM; one number: square blocks) -> the blocks; throws Error naming `what`
// on anything else.
inline DensityBlocks parse_density_film(const std::string& s, const char* what = "GOL_DENSITY_FILM") {
    long long v[2] = {0, 0};
    char tail = 0;
    const int n = sscanf(s.c_str(), " %lld , %lld %c", &v[0], &v[1], &tail);
    if (n == 2) return DensityBlocks{true, v[0], v[1]};
    if (n == 1 && sscanf(s.c_str(), " %lld %c", &v[0], &tail) == 1) return DensityBlocks{true, v[0], v[0]};
    throw Error(std::string(what) + " must be block_rows[,block_cols] (got '" + s + "')");
}

// The grid of a block shape on an H x W board (block_rows >= 1, block_cols a positive multiple of 64).
struct DensityGeo {
    i64 block_rows = 0, block_words = 0;  // rows and board words of a block
    i64 grid_rows = 0, grid_cols = 0;

    DensityGeo() = default;
    DensityGeo(const DensityBlocks& b, i64 H, i64 W)
        : block_rows(b.rows), block_words(b.cols / 64), grid_rows(ceil_div(H, b.rows)), grid_cols(ceil_div(W, b.cols)) {}
    i64 blocks() const { return grid_rows * grid_cols; }
    i64 slot_words() const { return (blocks() + 1) / 2; }  // u64 words of a generation's slot
};

}  // namespace gol
