// gol-mi355x: host API of the tensor kernels (tensor_kernels.hip): dense cells <-> packed words on the device.
#pragma once

#include <hip/hip_runtime.h>

#include "gol/cells.hpp"

namespace gol {
namespace hipk {

// k_cells_from_words<T>: the (n, rows, cols) cells of `s` (gol/cells.hpp; device words) as dense elements with the
// exact values 0 and 1 at dst.ptr (device memory).  Runs check_cells(s, dst) first: a description that reaches outside
// its words, or a buffer of another element count, throws before the launch.  Writes [ptr, ptr + numel) and nothing else.
void launch_cells_from_words(const CellSource& s, const CellBuffer& dst, hipStream_t stream);
// k_words_from_cells<T>: the (rows, cols) dense elements at src.ptr (device memory), alive iff != 0 (so -0.0 is dead
// and NaN alive), as split words into the rows of `t`: ceil(cols / 64) words per row, the last masked to the row's
// cells.  Runs check_cells(t, src) first.
void launch_words_from_cells(const CellBuffer& src, const CellTarget& t, hipStream_t stream);

// Throws Error unless [ptr, ptr + bytes) is device memory of `device` (hipPointerGetAttributes on both ends): the
// check the HIP backends run on a caller's pointer, so that a host or foreign pointer never reaches a kernel.
void require_device_pointer(const void* ptr, size_t bytes, int device, const char* what);

}  // namespace hipk
}  // namespace gol
