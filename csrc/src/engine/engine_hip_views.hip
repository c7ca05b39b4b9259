// gol-mi355x: HIP engine — windows, density maps and pattern stamping on the live board (view_kernels.hip).
//
// Readers first bring the canonical board up to date and drain the engine's streams, as tile_words() does;
// the stamp then refreshes ghosts and events exactly as set_tile_words() does.  Staging buffers grow on demand
// and are reused; an outgrown one is freed with the engine (hipFree may synchronise the whole device).
#include "../hip/tensor_kernels.hpp"
#include "hip_engine.hpp"

namespace gol {
namespace hipeng {

void HipEngine::grow_device(void** p, size_t* cap, size_t need) {
    if (need <= *cap) return;
    if (*p) deferred_free_.push_back(*p);
    *p = nullptr;
    *cap = 0;
    HIP_CHECK(hipMalloc(p, need));
    *cap = need;
}

u8* HipEngine::view_host(size_t need) {
    if (need > h_view_cap_) {
        if (h_view_) HIP_CHECK(hipHostFree(h_view_));
        h_view_ = nullptr;
        h_view_cap_ = 0;
        HIP_CHECK(hipHostMalloc((void**)&h_view_, need, hipHostMallocDefault));
        h_view_cap_ = need;
    }
    return h_view_;
}

void HipEngine::read_window_local(i64 r0, i64 c0, i64 rows, i64 cols, u8* out, i64 stride) {
    check_window(r0, c0, rows, cols);
    sync_canonical();
    synchronize();
    check_res_status();
    const std::vector<Piece> ps = pieces(g_, r0, c0, rows, cols);
    if (ps.empty()) return;
    std::vector<size_t> at;  // each piece dense, at a 256-byte boundary of the staging buffers
    size_t total = 0;
    for (const Piece& p : ps) {
        at.push_back(total);
        total += (size_t)round_up(p.rows * p.cols, 256);
    }
    grow_device((void**)&d_view_, &d_view_cap_, total);
    u8* host = view_host(total);
    for (size_t i = 0; i < ps.size(); ++i) {
        const Piece& p = ps[i];
        const size_t n = (size_t)(p.rows * p.cols);
        hipk::launch_window_bytes(view_buf(), L_, {p.tr, p.tc, p.rows, p.cols}, d_view_ + at[i], s_comp_);
        HIP_CHECK(hipGetLastError());
        // only the piece's bytes cross to the host
        HIP_CHECK(hipMemcpyAsync(host + at[i], d_view_ + at[i], n, hipMemcpyDeviceToHost, s_comp_));
        stats_.view_bytes_d2h += (u64)n;
    }
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    for (size_t i = 0; i < ps.size(); ++i) {
        const Piece& p = ps[i];
        for (i64 r = 0; r < p.rows; ++r)
            memcpy(out + (p.wr + r) * stride + p.wc, host + at[i] + (size_t)(r * p.cols), (size_t)p.cols);
    }
}

void HipEngine::density_local(i64 block_rows, i64 block_cols, u32* counts) {
    check_density(block_rows, block_cols);
    sync_canonical();
    synchronize();
    check_res_status();
    const i64 grows = ceil_div(g_.dec.H, block_rows), gcols = ceil_div(g_.dec.W, block_cols);
    const size_t bytes = (size_t)(grows * gcols) * sizeof(u32);
    grow_device((void**)&d_grid_, &d_grid_cap_, bytes);
    u32* host = reinterpret_cast<u32*>(view_host(bytes));
    HIP_CHECK(hipMemsetAsync(d_grid_, 0, bytes, s_comp_));
    hipk::launch_density(view_buf(), L_, g_.row0, g_.word0(), block_rows, block_cols / 64, gcols, d_grid_, s_comp_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host, d_grid_, bytes, hipMemcpyDeviceToHost, s_comp_));  // only the grid leaves the device
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    for (i64 i = 0; i < grows * gcols; ++i) counts[i] += host[i];
}

// One k_match launch over the canonical board.  The bitmap (keep) is a buffer in the board's layout, of which the
// kernel writes words 0 .. nw - 1 of rows 0 .. h - 1; only the counter comes to the host.
u64 HipEngine::match_local(const MatchTemplate& t, bool keep, bool or_into) {
    sync_canonical();
    synchronize();
    check_res_status();
    if (keep) grow_device((void**)&d_match_, &d_match_cap_, (size_t)L_.bytes());
    grow_device((void**)&d_match_cnt_, &d_match_cnt_cap_, 2 * sizeof(u64));
    u64* host = reinterpret_cast<u64*>(view_host(2 * sizeof(u64)));
    HIP_CHECK(hipMemsetAsync(d_match_cnt_, 0, 2 * sizeof(u64), s_comp_));
    hipk::launch_match(buf_[cur_], hipk::match_geo(L_, !dead_edges()), t, keep ? d_match_ : nullptr, or_into, nullptr,
                       d_match_cnt_, s_comp_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host, d_match_cnt_, sizeof(u64), hipMemcpyDeviceToHost, s_comp_));
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    return host[0];
}

void HipEngine::match_positions_local(i64 cap, std::vector<i32>* out) {
    if (cap < 1) return;
    if (!d_match_) throw Error("match: no bitmap to compact");
    const size_t bytes = (size_t)cap * 2 * sizeof(i32);
    grow_device((void**)&d_match_pos_, &d_match_pos_cap_, bytes);
    i32* host = reinterpret_cast<i32*>(view_host(bytes));
    HIP_CHECK(hipMemsetAsync(d_match_cnt_ + 1, 0, sizeof(u64), s_comp_));
    hipk::launch_match_positions(d_match_, hipk::match_geo(L_, !dead_edges()), d_match_pos_, cap, d_match_cnt_ + 1, s_comp_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host, d_match_pos_, bytes, hipMemcpyDeviceToHost, s_comp_));  // only the positions leave the device
    HIP_CHECK(hipStreamSynchronize(s_comp_));
    out->insert(out->end(), host, host + 2 * cap);
}

void HipEngine::match_bitmap_cells(const CellBuffer& dst) {
    if (!d_match_) throw Error("match: no bitmap to unpack");
    hipk::launch_cells_from_words(tile_source(d_match_, 0, 0, L_.h, L_.w), dst, s_comp_);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s_comp_));
}

// The objects of the canonical board.  Scratch (the parent array, four bytes per cell against the board's one bit, and
// the records) is allocated for the call and freed before it returns (hipk::run_components, run_component_labels):
// kept, the parent array would hold 32 times the board's bytes for the engine's lifetime for the sake of an occasional
// call.  Keeping it was not measured.
ComponentsResult HipEngine::components_local(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) {
    sync_canonical();
    synchronize();
    check_res_status();
    return hipk::run_components(buf_[cur_], hipk::match_geo(L_, !dead_edges()), nb, max_objects, hashes, want_records, s_comp_);
}

void HipEngine::components_labels_cells(CcNeighbourhood nb, void* dst, bool int64) {
    sync_canonical();
    synchronize();
    check_res_status();
    hipk::run_component_labels(buf_[cur_], hipk::match_geo(L_, !dead_edges()), nb, dst, int64, s_comp_);
}

void HipEngine::stamp_local(const RlePattern& p, i64 r0, i64 c0, StampMode mode) {
    check_stamp(p, r0, c0);
    sync_canonical();
    synchronize();
    check_res_status();
    const std::vector<Piece> ps = pieces(g_, r0, c0, p.rows, p.cols);
    if (ps.empty()) return;  // none of the pattern's cells is this rank's: its halos follow with the next exchange
    sub_current_ = false;    // the canonical board is edited: sub-tiles reload at the next run()
    canon_stale_ = false;
    const size_t bytes = p.words.size() * sizeof(u64);
    grow_device((void**)&d_pat_, &d_pat_cap_, bytes);
    upload(d_pat_, p.words.data(), bytes);
    for (const Piece& q : ps) {
        hipk::launch_stamp(buf_[cur_], L_, {q.tr, q.tc, q.rows, q.cols}, d_pat_, p.nw(), q.wr, q.wc, (int)mode, s_comp_);
        HIP_CHECK(hipGetLastError());
    }
    post(buf_[cur_], s_comp_);
    mark_ready();
    synchronize();
}

}  // namespace hipeng
}  // namespace gol
