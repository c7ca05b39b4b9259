// gol-mi355x: HIP engine — dense cells on the device (engine.hpp: the tensor readers and writers; kernels:
// src/hip/tensor_kernels.hip).  The caller's pointer is device memory of this engine's device, verified before anything
// is launched.  Readers first bring the canonical board up to date and drain the engine's streams, as tile_words() does;
// the writer then refreshes ghosts and events exactly as set_tile_words() does.  Every call runs on the compute stream
// and synchronises it before returning.
#include "../hip/tensor_kernels.hpp"
#include "hip_engine.hpp"

namespace gol {
namespace hipeng {

void HipEngine::check_cell_pointer(const CellBuffer& b, const char* what) {
    if (b.numel < 1) throw Error(std::string(what) + ": the buffer is empty");
    hipk::require_device_pointer(b.ptr, (size_t)(b.numel * cell_size(b.type)), dev_, what);
}

void HipEngine::read_rect_cells(i64 r0, i64 c0, i64 rows, i64 cols, const CellBuffer& dst) {
    sync_canonical();
    synchronize();
    check_res_status();
    hipk::launch_cells_from_words(tile_source(view_buf(), r0, c0, rows, cols), dst, s_comp_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s_comp_));
}

void HipEngine::write_tile_cells_local(const CellBuffer& src) {
    CellTarget t;
    t.base = buf_[cur_] + L_.index(0, 0);
    t.words = L_.words() - L_.index(0, 0);
    t.row_stride = L_.pitch, t.rows = L_.h, t.cols = L_.w;
    check_cells(t, src, "write_tile_cells()");  // (before the board is given up)
    sub_current_ = false;  // the canonical board is rewritten: sub-tiles reload at the next run()
    canon_stale_ = false;
    synchronize();
    hipk::launch_words_from_cells(src, t, s_comp_);
    HIP_CHECK(hipGetLastError());
    post(buf_[cur_], s_comp_);
    mark_ready();
    synchronize();
}

// The chunk's frames are slots 0 .. frames - 1 of the device record (run_film_cells() starts from an empty record and
// drains after every run() of at most film_cap_ generations): unpacked at their frame offset, then zeroed where they
// are, as census_collect() leaves them, and nothing goes to film_host_.
void HipEngine::film_drain_cells(size_t frames, const CellBuffer& dst, size_t at) {
    if (frames == 0) return;
    if (!d_census_ || census_dev_n_ != frames || frames > census_cap_)
        throw Error(strprintf("run_film_cells(): the device record holds %zu frames, the chunk has %zu", census_dev_n_, frames));
    synchronize();  // the passes of either stream have stored their words
    const i64 per = film_geo_.rows * film_geo_.cols;
    CellBuffer part{(u8*)dst.ptr + at * (size_t)(per * cell_size(dst.type)), dst.type, (i64)frames * per};
    hipk::launch_cells_from_words(film_source(d_census_, (i64)(census_cap_ * slot_words()), (i64)frames), part, s_comp_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemsetAsync(d_census_, 0, frames * slot_bytes(), s_comp_));
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    census_dev_n_ = 0;
}

}  // namespace hipeng
}  // namespace gol
