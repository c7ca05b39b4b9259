// gol-mi355x: the HIP backend of soup batches (soups.hpp): device memory for the per-soup state and the launches of
// step_soups (src/hip/soup_kernel.hip).  One stream; after every settle / transient launch the host reads one counter,
// so launches never queue up unbounded.
#include "../hip/soup_kernel.hpp"
#include "../hip/tensor_kernels.hpp"
#include "gol/engine.hpp"
#include "hip_engine.hpp"

namespace gol {

namespace {

class HipSoups final : public SoupBatch {
   public:
    explicit HipSoups(const SoupConfig& c) : SoupBatch(c), wps_(words_per_soup()) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) throw Error("soups: backend hip needs a HIP device, none found");
        if (c.device < 0 || c.device >= count)
            throw Error(strprintf("soups: device %d is outside 0 .. %d", c.device, count - 1));
        if (cfg_.workgroup == 0) {
            const long long wg = env_int("GOL_SOUPS_WG", 64);
            if (wg != 64 && wg != 128 && wg != 256) throw Error(strprintf("GOL_SOUPS_WG=%lld is not 64, 128 or 256", wg));
            cfg_.workgroup = (int)wg;
        }
        HIP_CHECK(hipSetDevice(cfg_.device));
        HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        try {
            HIP_CHECK(hipMalloc(&board_, bytes()));
            HIP_CHECK(hipMalloc(&state_, (size_t)cfg_.n * sizeof(SoupState)));
            HIP_CHECK(hipMalloc(&counters_, 2 * sizeof(u32)));
        } catch (...) {
            release();
            throw;
        }
    }
    ~HipSoups() override { release(); }

    void synchronize() override {
        use();
        HIP_CHECK(hipStreamSynchronize(stream_));
    }

   protected:
    void do_init_seed(u64 seed) override {
        use();
        hipk::launch_init_soups(m(), board_, state_, (u32)cfg_.n, seed, stream_);
        reset();
    }
    void do_upload(const u64* split) override {
        use();
        HIP_CHECK(hipMemcpyAsync(board_, split, bytes(), hipMemcpyHostToDevice, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));  // (the caller's buffer is free again)
        hipk::launch_reset_soup_states(state_, (u32)cfg_.n, stream_);
        reset();
    }
    void do_plain(u32 gens) override {
        use();
        hipk::launch_step_soups(m(), hipk::SOUP_PLAIN, cfg_.rule, args(gens, 0), cfg_.workgroup, stream_);
    }
    void do_begin_search() override {
        use();
        if (!saved_) HIP_CHECK(hipMalloc(&saved_, bytes()));
        if (!init_) HIP_CHECK(hipMalloc(&init_, bytes()));
        HIP_CHECK(hipMemcpyAsync(saved_, board_, bytes(), hipMemcpyDeviceToDevice, stream_));
        HIP_CHECK(hipMemcpyAsync(init_, board_, bytes(), hipMemcpyDeviceToDevice, stream_));
        hipk::launch_begin_soup_search(state_, (u32)cfg_.n, stream_);
    }
    u64 do_settle(u32 gens, u32 max_gens) override {
        use();
        hipk::launch_step_soups(m(), hipk::SOUP_SETTLE, cfg_.rule, args(gens, max_gens), cfg_.workgroup, stream_);
        return counter(0);
    }
    u64 do_transient(u32 gens) override {
        use();
        if (!tmp_) HIP_CHECK(hipMalloc(&tmp_, bytes()));
        HIP_CHECK(hipMemsetAsync(counters_ + 1, 0, sizeof(u32), stream_));
        hipk::launch_step_soups(m(), hipk::SOUP_TRANSIENT, cfg_.rule, args(gens, 0), cfg_.workgroup, stream_);
        return counter(1);
    }
    void do_fetch_states(SoupState* out) override {
        use();
        HIP_CHECK(hipMemcpyAsync(out, state_, (size_t)cfg_.n * sizeof(SoupState), hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    void do_fetch_board(i64 soup, u64* split) override {
        use();
        const size_t one = (size_t)wps_ * sizeof(u64);
        HIP_CHECK(hipMemcpyAsync(split, board_ + (size_t)soup * (size_t)wps_, one, hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    // dense cells on the device (tensor_kernels.hip): the caller's pointer is verified before anything is launched
    void do_read_cells(i64 first, i64 count, const CellBuffer& dst) override {
        use();
        hipk::require_device_pointer(dst.ptr, (size_t)(dst.numel * cell_size(dst.type)), cfg_.device, "soups: read_boards_cells()");
        hipk::launch_cells_from_words(soup_source(board_, first, count), dst, stream_);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    void do_init_cells(const CellBuffer& src) override {
        use();
        hipk::require_device_pointer(src.ptr, (size_t)(src.numel * cell_size(src.type)), cfg_.device, "soups: init_cells()");
        hipk::launch_words_from_cells(src, soup_target(board_), stream_);
        HIP_CHECK(hipGetLastError());
        hipk::launch_reset_soup_states(state_, (u32)cfg_.n, stream_);
        reset();
    }
    // k_match (src/hip/match_kernel.hip) over the store: n dense tori of S rows x m words, one counter per soup
    void do_match_counts(const std::vector<MatchTemplate>& oriented, u32* counts) override {
        use();
        HIP_CHECK(hipStreamSynchronize(stream_));
        if (!match_counts_) HIP_CHECK(hipMalloc(&match_counts_, (size_t)cfg_.n * sizeof(u32)));
        hipk::MatchGeo g;
        g.base = 0, g.pitch = m(), g.batch_stride = wps_;
        g.w = cfg_.size, g.h = (i32)cfg_.size, g.nw = m();
        g.torus = 1, g.batch = (i32)cfg_.n;
        HIP_CHECK(hipMemsetAsync(match_counts_, 0, (size_t)cfg_.n * sizeof(u32), stream_));
        for (const MatchTemplate& t : oriented) {
            hipk::launch_match(board_, g, t, nullptr, false, match_counts_, nullptr, stream_);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipMemcpyAsync(counts, match_counts_, (size_t)cfg_.n * sizeof(u32), hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    // the kernels of src/hip/components_kernel.hip over the store, as k_match sees it
    ComponentsResult do_components(CcNeighbourhood nb, i64 max_objects, bool hashes, bool want_records) override {
        use();
        HIP_CHECK(hipStreamSynchronize(stream_));
        hipk::MatchGeo g;
        g.base = 0, g.pitch = m(), g.batch_stride = wps_;
        g.w = cfg_.size, g.h = (i32)cfg_.size, g.nw = m();
        g.torus = 1, g.batch = (i32)cfg_.n;
        return hipk::run_components(board_, g, nb, max_objects, hashes, want_records, stream_);
    }

   private:
    size_t bytes() const { return (size_t)cfg_.n * (size_t)wps_ * sizeof(u64); }
    void use() { HIP_CHECK(hipSetDevice(cfg_.device)); }
    // a new set of boards: the population of generation 0 (a launch of no generations), no soup settled
    void reset() {
        HIP_CHECK(hipMemsetAsync(counters_, 0, 2 * sizeof(u32), stream_));
        hipk::launch_step_soups(m(), hipk::SOUP_PLAIN, cfg_.rule, args(0, 0), cfg_.workgroup, stream_);
        HIP_CHECK(hipStreamSynchronize(stream_));
    }
    hipk::SoupArgs args(u32 gens, u32 max_gens) const {
        hipk::SoupArgs a;
        a.board = board_;
        a.saved = saved_;
        a.init = init_;
        a.tmp = tmp_;
        a.state = state_;
        a.counters = counters_;
        a.n = (u32)cfg_.n;
        a.gens = gens;
        a.max_gens = max_gens;
        return a;
    }
    u64 counter(int i) {
        u32 v = 0;
        HIP_CHECK(hipMemcpyAsync(&v, counters_ + i, sizeof(u32), hipMemcpyDeviceToHost, stream_));
        HIP_CHECK(hipStreamSynchronize(stream_));
        return v;
    }
    void release() {
        for (void* p : {(void*)board_, (void*)saved_, (void*)init_, (void*)tmp_, (void*)state_, (void*)counters_, (void*)match_counts_})
            if (p) (void)hipFree(p);
        match_counts_ = nullptr;
        board_ = saved_ = init_ = tmp_ = nullptr;
        state_ = nullptr;
        counters_ = nullptr;
        if (stream_) (void)hipStreamDestroy(stream_);
        stream_ = nullptr;
    }

    i64 wps_;
    hipStream_t stream_ = nullptr;
    u64 *board_ = nullptr, *saved_ = nullptr, *init_ = nullptr, *tmp_ = nullptr;
    SoupState* state_ = nullptr;
    u32* counters_ = nullptr;
    u32* match_counts_ = nullptr;  // match_counts(): one counter per soup, allocated on first use
};

}  // namespace

std::unique_ptr<SoupBatch> make_hip_soups(const SoupConfig& c) { return std::make_unique<HipSoups>(c); }

}  // namespace gol
