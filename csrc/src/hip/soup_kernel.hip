// gol-mi355x: step_soups<M, GENERIC, MODE> -- many small tori per launch, one wave64 per soup, for gfx950 (CDNA4).
//
// A soup is a square torus of side S = 64 M.  Its wave keeps the whole board in registers for a launch: lane l holds
// rows M l .. M l + M - 1, each as M words in split format (bits.hpp: lo = even columns, hi = odd columns), so
//   * the left / right neighbours of a word half come from one funnel shift (v_alignbit_b32) with the neighbouring
//     word of the same row, which is in the same lane; at M = 1 that word is the word itself and the funnel shift is
//     a rotate: the torus's x-wrap costs nothing;
//   * the rows above a lane's first row and below its last row come from the neighbouring lanes by one DPP lane
//     rotate of the four horizontal-sum planes (wave_ror:1 / wave_rol:1: lane 0 <-> lane 63 is the torus's y-wrap);
//   * hsum_split's gates (2 x xor3 + 2 x maj per word) and rule32 (B3/S23, 7 gates per word half) or
//     RuleGates::rule (any Moore rule from run-time masks, 24 gates) finish a generation.
// No load, store, LDS access or barrier happens between a launch's first and last generation.  The code rests on
// warpSize == 64.
//
// MODE (soup_kernel.hpp):
//   SOUP_PLAIN      gens generations, no comparison.
//   SOUP_SETTLE     Brent's search (soups.hpp): after every generation the board is compared with the saved copy
//                   (xor / or over the lane's words, one ballot: every branch on it is wave-uniform); a settled
//                   soup's wave ends.  At most gens generations per launch and never past max_gens.
//   SOUP_TRANSIENT  the two-copy walk from the initial board that finds a settled soup's exact transient; at most
//                   gens loop passes per launch.
// The state of a soup (SoupState) is wave-uniform: read with scalar loads, written by lane 0.  The population is
// counted once, when the wave stops (v_bcnt_u32_b32 per word half and one wave reduction).
//
// Registers and instruction counts of the gfx950 code: docs/PERFORMANCE.md section 27.
#include <cstddef>
#include <type_traits>

#include "rule_runner.hpp"
#include "soup_kernel.hpp"

namespace gol {
namespace hipk {

namespace {

static_assert(sizeof(SoupState) == 32, "SoupState is read and written as eight dwords");

template <int M>
struct Soup {
    u32 lo[M][M], hi[M][M];  // [row of the lane][word]
};

template <int M>
__device__ __forceinline__ void load_soup(Soup<M>& b, const u64* __restrict__ p) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const u64 v = p[i * M + j];
            b.lo[i][j] = (u32)v;
            b.hi[i][j] = (u32)(v >> 32);
        }
}

template <int M>
__device__ __forceinline__ void store_soup(const Soup<M>& b, u64* __restrict__ p) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) p[i * M + j] = (u64)b.lo[i][j] | ((u64)b.hi[i][j] << 32);
}

// true when the two boards are the same in every lane (wave-uniform)
template <int M>
__device__ __forceinline__ bool same_soup(const Soup<M>& a, const Soup<M>& b) {
    u32 diff = 0;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) diff |= (a.lo[i][j] ^ b.lo[i][j]) | (a.hi[i][j] ^ b.hi[i][j]);
    return __builtin_amdgcn_ballot_w64(diff != 0) == 0;
}

template <int M>
__device__ __forceinline__ u32 soup_population(const Soup<M>& b) {
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) c += __popc(b.lo[i][j]) + __popc(b.hi[i][j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    return c;
}

// hsum_split with the neighbouring words in the lane: ph = the previous word's odd half, nl = the next word's even half.
__device__ __forceinline__ void hsum_words(u32 lo, u32 hi, u32 ph, u32 nl, u32& s0lo, u32& s1lo, u32& s0hi, u32& s1hi) {
    const u32 Le = __builtin_amdgcn_alignbit(hi, ph, 31);  // (hi << 1) | (ph >> 31)
    const u32 Ro = __builtin_amdgcn_alignbit(nl, lo, 1);   // (lo >> 1) | (nl << 31)
    s0lo = b3<kLutXor3>(Le, lo, hi);
    s1lo = b3<kLutMaj>(Le, lo, hi);
    s0hi = b3<kLutXor3>(lo, hi, Ro);
    s1hi = b3<kLutMaj>(lo, hi, Ro);
}

struct ConwayFinish {
    __device__ __forceinline__ explicit ConwayFinish(const RuleMasks&) {}
    __device__ __forceinline__ u32 rule(u32 a0, u32 a1, u32 b0, u32 b1, u32 c0, u32 c1, u32 x) const {
        return rule32(a0, a1, b0, b1, c0, c1, x);
    }
};

// One generation of the wave's torus, in place.  Rows 0 and M + 1 of the sum planes are the neighbouring lanes'.
template <int M, typename Finish>
__device__ __forceinline__ void step_soup(Soup<M>& b, const Finish& f) {
    u32 s[M + 2][M][4];  // s0 lo, s1 lo, s0 hi, s1 hi
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j)
            hsum_words(b.lo[i][j], b.hi[i][j], b.hi[i][(j + M - 1) % M], b.lo[i][(j + 1) % M], s[i + 1][j][0], s[i + 1][j][1],
                       s[i + 1][j][2], s[i + 1][j][3]);
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[0][j][q] = dpp_ring_prev(s[M][j][q]);      // the last row of the lane above
            s[M + 1][j][q] = dpp_ring_next(s[1][j][q]);  // the first row of the lane below
        }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            b.lo[i][j] = f.rule(s[i][j][0], s[i][j][1], s[i + 1][j][0], s[i + 1][j][1], s[i + 2][j][0], s[i + 2][j][1], b.lo[i][j]);
            b.hi[i][j] = f.rule(s[i][j][2], s[i][j][3], s[i + 1][j][2], s[i + 1][j][3], s[i + 2][j][2], s[i + 2][j][3], b.hi[i][j]);
        }
}

// SoupState in registers (wave-uniform), in the struct's order.
struct SoupRegs {
    u32 g, s, w, period, population, flags, tadv, tcount;
    __device__ __forceinline__ void store(uint4* p) const {
        p[0] = make_uint4(g, s, w, period);
        p[1] = make_uint4(population, flags, tadv, tcount);
    }
};
static_assert(offsetof(SoupState, period) == 12 && offsetof(SoupState, population) == 16 && offsetof(SoupState, tcount) == 28,
              "SoupRegs follows SoupState");

template <int M, bool GENERIC, int MODE>
__global__ __launch_bounds__(256) void step_soups(SoupArgs a, RuleMasks rm) {
    const u32 soup = (u32)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (soup >= a.n) return;  // (uniform: the last workgroup's spare waves)
    const u32 lane = threadIdx.x & 63u;
    const size_t off = ((size_t)soup * 64u + lane) * (size_t)(M * M);
    const std::conditional_t<GENERIC, RuleGates, ConwayFinish> f(rm);
    // (the state travels as two dwordx4, field by field: copied as a struct, its untouched fields went through LDS)
    uint4* const sp = reinterpret_cast<uint4*>(a.state + soup);
    const uint4 q0 = sp[0], q1 = sp[1];
    SoupRegs st{q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};

    if constexpr (MODE == SOUP_PLAIN) {
        Soup<M> b;
        load_soup(b, a.board + off);
        for (u32 k = 0; k < a.gens; ++k) step_soup(b, f);
        store_soup(b, a.board + off);
        st.g += a.gens;
        st.population = soup_population(b);
        if (lane == 0) st.store(sp);
    } else if constexpr (MODE == SOUP_SETTLE) {
        if (st.period != 0 || st.g >= a.max_gens) return;
        Soup<M> b, sv;
        load_soup(b, a.board + off);
        load_soup(sv, a.saved + off);
        const u32 left = a.max_gens - st.g;
        const u32 end = st.g + (a.gens < left ? a.gens : left);
        while (st.g < end) {
            step_soup(b, f);
            ++st.g;
            if (same_soup(b, sv)) {
                st.period = st.g - st.s;
                break;
            }
            if (st.g - st.s == st.w) {
                sv = b;
                st.s = st.g;
                st.w <<= 1;
            }
        }
        store_soup(b, a.board + off);
        store_soup(sv, a.saved + off);
        st.population = soup_population(b);
        if (lane == 0) {
            st.store(sp);
            if (st.period != 0) atomicAdd(a.counters + 0, 1u);
        }
    } else {
        if (st.period == 0 || (st.flags & kSoupTransientDone)) return;
        Soup<M> x, y;  // x from the initial board, y the period ahead of it
        if (!(st.flags & kSoupTransientStarted)) {
            load_soup(x, a.init + off);
            y = x;
            st.flags |= kSoupTransientStarted;
            st.tadv = st.tcount = 0;
        } else {
            load_soup(x, a.saved + off);
            load_soup(y, a.tmp + off);
        }
        for (u32 k = 0; k < a.gens; ++k) {
            if (st.tadv < st.period) {
                step_soup(y, f);
                ++st.tadv;
                continue;
            }
            if (same_soup(x, y)) {
                st.flags |= kSoupTransientDone;
                break;
            }
            step_soup(x, f);
            step_soup(y, f);
            ++st.tcount;
        }
        store_soup(x, a.saved + off);
        store_soup(y, a.tmp + off);
        if (lane == 0) {
            st.store(sp);
            if (!(st.flags & kSoupTransientDone)) atomicAdd(a.counters + 1, 1u);
        }
    }
}

template <int M, bool GENERIC>
const void* soup_kernel_mode(SoupMode mode) {
    switch (mode) {
        case SOUP_PLAIN: return (const void*)step_soups<M, GENERIC, SOUP_PLAIN>;
        case SOUP_SETTLE: return (const void*)step_soups<M, GENERIC, SOUP_SETTLE>;
        default: return (const void*)step_soups<M, GENERIC, SOUP_TRANSIENT>;
    }
}

const void* soup_kernel_of(int m, bool generic, SoupMode mode) {
    switch (m) {
        case 1: return generic ? soup_kernel_mode<1, true>(mode) : soup_kernel_mode<1, false>(mode);
        case 2: return generic ? soup_kernel_mode<2, true>(mode) : soup_kernel_mode<2, false>(mode);
        case 4: return generic ? soup_kernel_mode<4, true>(mode) : soup_kernel_mode<4, false>(mode);
        default: return nullptr;
    }
}

__global__ __launch_bounds__(256) void k_init_soups(u64* __restrict__ board, u64 words, u32 m, u64 seed) {
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= words) return;
    const u64 per = 64ull * m * m;  // words of a soup
    const u64 soup = i / per, rem = i % per;
    board[i] = split_word(random_word(seed + soup, (i64)(rem / m), (i64)(rem % m), (i64)m));
}

__global__ __launch_bounds__(256) void k_reset_soup_states(SoupState* __restrict__ state, u32 n, u32 keep_g) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    SoupState st;
    if (keep_g) {  // the search begins here
        st = state[i];
        st.s = st.g;
        st.w = 1;
    }
    state[i] = st;
}

void check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw Error(strprintf("%s launch failed: %s", what, hipGetErrorString(e)));
}

}  // namespace

void launch_step_soups(int m, SoupMode mode, const Rule& rule, const SoupArgs& a, int workgroup, hipStream_t stream) {
    if (rule.nbhd != Nbhd::Moore || (rule.birth & 1u) || rule.birth > 0x1FFu || rule.survive > 0x1FFu)
        throw Error("step_soups: rule " + rule.str() + " is no B0-free Moore rule");
    if (workgroup != 64 && workgroup != 128 && workgroup != 256)
        throw Error(strprintf("step_soups: workgroup %d is not 64, 128 or 256", workgroup));
    if (a.n < 1 || (i64)a.n > kSoupsMax) throw Error(strprintf("step_soups: n = %u is outside 1 .. 2^20", a.n));
    const void* f = soup_kernel_of(m, !rule.is_conway(), mode);
    if (!f) throw Error(strprintf("step_soups: no kernel for soups of side %d", 64 * m));
    const unsigned waves = (unsigned)workgroup / 64u;
    SoupArgs args = a;
    RuleMasks rm{rule.birth, rule.survive};
    void* kargs[] = {&args, &rm};
    const hipError_t e = hipLaunchKernel(f, dim3((a.n + waves - 1) / waves), dim3((unsigned)workgroup), kargs, 0, stream);
    if (e != hipSuccess) throw Error(strprintf("step_soups launch failed: %s", hipGetErrorString(e)));
}

void launch_init_soups(int m, u64* board, SoupState* state, u32 n, u64 seed, hipStream_t stream) {
    const u64 words = (u64)n * 64u * (u64)(m * m);
    hipLaunchKernelGGL(k_init_soups, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, stream, board, words, (u32)m, seed);
    check_launch("init_soups");
    launch_reset_soup_states(state, n, stream);
}

void launch_reset_soup_states(SoupState* state, u32 n, hipStream_t stream) {
    hipLaunchKernelGGL(k_reset_soup_states, dim3((n + 255) / 256), dim3(256), 0, stream, state, n, 0u);
    check_launch("reset_soup_states");
}

void launch_begin_soup_search(SoupState* state, u32 n, hipStream_t stream) {
    hipLaunchKernelGGL(k_reset_soup_states, dim3((n + 255) / 256), dim3(256), 0, stream, state, n, 1u);
    check_launch("begin_soup_search");
}

}  // namespace hipk
}  // namespace gol
