// gol-mi355x: what the launchers of the four generic-rule kernels (rule_runner.hpp) share on the host: the argument
// checks, the TileArgs fill, the depth and row-mode dispatch, the occupancy query and the launch itself.  `kernel`
// in the checks is the kernel's name as the error messages print it.
#pragma once

#include <algorithm>
#include <type_traits>

#include "rule_runner.hpp"

namespace gol {
namespace hipk {

// The von Neumann and hexagonal instantiations of the four kernels (nbhd_rule_kernel.hip, nbhd_bounded_kernel.hip,
// nbhd_census_kernel.hip, nbhd_signature_kernel.hip; the gates: nbhd_gates.hpp), units of their own so that they
// build beside the Moore units and leave those objects alone.  nullptr: depth k is not instantiated.
const void* nbhd_rule_kernel(Nbhd nbhd, int k, u32 flags);
const void* nbhd_bounded_kernel(Nbhd nbhd, int k, u32 flags);
const void* nbhd_census_kernel(Nbhd nbhd, int k, u32 flags, bool bounded);
const void* nbhd_signature_kernel(Nbhd nbhd, int k, u32 flags, bool bounded);
const void* nbhd_film_kernel(Nbhd nbhd, int k, u32 flags, bool bounded);  // (step_film: nbhd_film_kernel.hip)
const void* nbhd_density_kernel(Nbhd nbhd, int k, u32 flags, bool bounded);  // (step_density: nbhd_density_kernel.hip)
const void* nbhd_envelope_kernel(Nbhd nbhd, int k, u32 flags, bool bounded);  // (step_envelope: nbhd_envelope_kernel.hip)

namespace {

constexpr int kMaxRuleDepth = 8;  // depths K = 1 .. 8 are instantiated: every remainder of a superstep is one pass

// The masks within the neighbourhood's range of counts (8, von Neumann 4, hexagonal 6).
inline void check_rule_masks(const char* kernel, const Rule& rule) {
    if ((unsigned)rule.nbhd > (unsigned)Nbhd::Hex) throw Error(strprintf("%s: unknown neighbourhood %u", kernel, (unsigned)rule.nbhd));
    const int top = nbhd_max_count(rule.nbhd);
    const u32 all = (2u << top) - 1u;
    if ((rule.birth & 1u) || rule.birth > all || rule.survive > all)
        throw Error(strprintf("%s: rule masks outside B1..%d / S0..%d (B0 is out of scope)", kernel, top, top));
}

inline void check_place(const char* kernel, const BoardEdges& e) {
    if (e.rows < 1 || e.cols < 1 || e.row0 < 0 || e.row0 >= e.rows || e.word0 < 0 || e.word0 >= ceil_div(e.cols, 64))
        throw Error(strprintf("%s: tile at row %lld, word %lld outside the %lld x %lld board", kernel, (long long)e.row0,
                              (long long)e.word0, (long long)e.rows, (long long)e.cols));
}

inline void check_tile_cols(const char* kernel, i64 tile_cols, const StepParams& p) {
    if (tile_cols < 1 || ceil_div(tile_cols, 64) != (i64)p.nw)
        throw Error(strprintf("%s: a tile of %lld columns does not have %d words", kernel, (long long)tile_cols, (int)p.nw));
}

// place == nullptr: no place on a board (the torus census; the fields stay 0).  tile_cols == 0: no own cells
// (step_rule_bounded).
inline TileArgs tile_args(const BoardEdges* place, i64 tile_cols, const StepParams& p) {
    TileArgs ta{};
    if (place) {
        const i64 gwords = ceil_div(place->cols, 64);
        const u64 tail = storage_mask(gwords - 1, place->cols);
        ta = TileArgs{place->row0, place->rows, place->word0, gwords, (u32)tail, (u32)(tail >> 32), 0, 0};
    }
    if (tile_cols > 0) {
        const u64 own = storage_mask((i64)p.nw - 1, tile_cols);
        ta.own_lo = (u32)own;
        ta.own_hi = (u32)(own >> 32);
    }
    return ta;
}

// The instantiation of a kernel template for depth k and the row mode of flags, nullptr when k is not instantiated:
// kernel(K, ROWS) returns the address of the kernel's <K, ROWS, ...> from two std::integral_constant.
template <class F>
const void* kernel_of(int k, u32 flags, F kernel) {
    const std::integral_constant<int, ROWS_WRAP> wrap{};
    const std::integral_constant<int, ROWS_GHOST> ghost{};
    const bool wy = flags & STEP_WRAP_Y;
    switch (k) {
#define DEPTH_CASE(K)                                           \
    case K: {                                                   \
        const std::integral_constant<int, K> depth{};           \
        return wy ? kernel(depth, wrap) : kernel(depth, ghost); \
    }
        DEPTH_CASE(1) DEPTH_CASE(2) DEPTH_CASE(3) DEPTH_CASE(4) DEPTH_CASE(5) DEPTH_CASE(6) DEPTH_CASE(7) DEPTH_CASE(8)
#undef DEPTH_CASE
        default:
            return nullptr;
    }
}

// Resident 256-thread workgroups per CU of kernel f (1 when it cannot be asked).
inline int blocks_per_cu(const void* f) {
    int nb = 0;
    if (!f || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, f, 64 * kWavesPerBlock, 0) != hipSuccess || nb < 1) return 1;
    return std::min(nb, 32 / kWavesPerBlock);
}

// Launch f over the waves of plan: the arguments every generic-rule kernel begins with, then `more` in order.
// `what` names the kernel in the error message.
template <class... A>
void launch_generic(const char* what, const void* f, const Rule& rule, const u64* src, u64* dst, const LaneDesc* plan,
                    i64 n_waves, const StepParams& p, hipStream_t s, A... more) {
    const dim3 grid((unsigned)(n_waves / kWavesPerBlock)), block(64 * kWavesPerBlock);
    StepParams pp = p;
    if (!pp.trash) pp.trash = trash_of_current_device();
    RuleMasks rm{rule.birth, rule.survive};
    void* args[] = {(void*)&src, (void*)&dst, (void*)&plan, (void*)&pp, (void*)&rm, (void*)&more...};
    hipError_t e = hipLaunchKernel(f, grid, block, args, 0, s);
    if (e != hipSuccess) throw Error(strprintf("%s kernel launch failed: %s", what, hipGetErrorString(e)));
}

}  // namespace
}  // namespace hipk
}  // namespace gol
