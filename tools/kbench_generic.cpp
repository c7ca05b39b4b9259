// Standalone timing harness for step_census and step_signature at kernel level: every instantiation (depth 1 .. 8,
// ghost or wrap rows, torus or dead edges) on one tile that is the whole board, balanced one-round plan, rule
// B36/S23.  The engine on one GPU launches the wrap-row kernels only; this launches the ghost-row ones too (their
// ghost rows are not exchanged: the board's values are meaningless, only the time is).  Links against a tree's
// libgolcore.a, so the same source times two trees (docs/PERFORMANCE.md section 23):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I<tree>/csrc/include -c tools/kbench_generic.cpp -o kbench_generic.o
//   hipcc kbench_generic.o <tree>/build/libgolcore.a -L/opt/rocm/lib -lrccl -fopenmp -o <tree>/build/kbench_generic
//   <tree>/build/kbench_generic [N=8192] [gens=960] [reps=5] [label]
// One line per instantiation: the median, minimum and maximum of `reps` timed runs of `gens` generations after one
// warm-up run, in us per generation (HIP events around the launches of a run).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <vector>

#include "gol/hip_kernels.hpp"
#include "gol/plan.hpp"
#include "gol/rule.hpp"

using namespace gol;

#define CK(x)                                                      \
    do {                                                           \
        hipError_t e = (x);                                        \
        if (e != hipSuccess) {                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); \
            exit(1);                                               \
        }                                                          \
    } while (0)

int main(int argc, char** argv) try {
    const i64 N = argc > 1 ? atoll(argv[1]) : 8192;
    const int gens = argc > 2 ? atoi(argv[2]) : 960;
    const int reps = argc > 3 ? atoi(argv[3]) : 5;
    const char* label = argc > 4 ? argv[4] : "tree";
    constexpr int kMaxK = 8;
    Layout L(N, N, kMaxK);
    const size_t bytes = (size_t)(L.words() + hipk::kSlackRows * L.pitch) * 8;
    u64 *a, *b, *slots;
    CK(hipMalloc(&a, bytes));
    CK(hipMalloc(&b, bytes));
    CK(hipMemset(a, 0, bytes));
    CK(hipMemset(b, 0, bytes));
    const size_t slot_bytes = (size_t)kMaxK * std::max(hipk::kCensusSlotWords, hipk::kSigSlotWords) * 8;
    CK(hipMalloc(&slots, slot_bytes));
    CK(hipMemset(slots, 0, slot_bytes));
    hipk::launch_init_fill(a, L, hipk::InitParams{0, 0, L.nw, 0x5EED, 2}, 0);
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    hipk::ensure_trash();
    const Rule rule = Rule::parse("B36/S23");
    const hipk::BoardEdges place{0, N, 0, N};
    const std::vector<Region> rg = {{0, N, 0, L.nw}};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int sig = 0; sig < 2; ++sig)
        for (int dead = 0; dead < 2; ++dead)
            for (int wrap = 0; wrap < 2; ++wrap)
                for (int K = 1; K <= kMaxK; ++K) {
                    const u32 flags = wrap ? hipk::STEP_WRAP_Y : 0u;
                    const bool xwrap = !dead;  // (a bounded board's plans are built without x-wrap)
                    const i64 bpc = sig ? hipk::signature_blocks_per_cu(K, flags, dead) : hipk::census_blocks_per_cu(K, flags, dead);
                    const i64 rows = balanced_rows_per_chunk(rg, L.nw, N, K, bpc * kWavesPerBlock * prop.multiProcessorCount,
                                                             2 * K, xwrap);
                    PlanStats st;
                    const std::vector<LaneDesc> lanes = build_plan(rg, L.nw, N, rows, K, xwrap, &st);
                    const std::string bad = validate_plan(lanes, L.nw, N, L.R, K, wrap != 0);
                    if (!bad.empty()) {
                        fprintf(stderr, "unsafe plan: %s\n", bad.c_str());
                        return 1;
                    }
                    LaneDesc* dplan;
                    CK(hipMalloc(&dplan, lanes.size() * sizeof(LaneDesc)));
                    CK(hipMemcpy(dplan, lanes.data(), lanes.size() * sizeof(LaneDesc), hipMemcpyHostToDevice));
                    const hipk::StepParams sp{L.pitch, (i32)L.h, (i32)L.nw, L.R, flags};
                    const int steps = std::max(1, gens / K);
                    std::vector<float> us;
                    for (int rep = 0; rep <= reps; ++rep) {
                        CK(hipDeviceSynchronize());
                        CK(hipEventRecord(e0, 0));
                        for (int s = 0; s < steps; ++s) {
                            if (sig)
                                hipk::launch_step_signature(K, rule, place, dead, L.w, a, b, dplan, st.waves, sp, slots, 0);
                            else
                                hipk::launch_step_census(K, rule, dead ? &place : nullptr, L.w, a, b, dplan, st.waves, sp, slots, 0);
                            std::swap(a, b);
                        }
                        CK(hipEventRecord(e1, 0));
                        CK(hipEventSynchronize(e1));
                        float ms = 0;
                        CK(hipEventElapsedTime(&ms, e0, e1));
                        if (rep > 0) us.push_back(ms * 1e3f / (steps * K));
                    }
                    CK(hipGetLastError());
                    CK(hipFree(dplan));
                    std::sort(us.begin(), us.end());
                    printf("%s %s K=%d %s %s rows %lld waves %lld blocks_per_cu %d us/gen median %.4f min %.4f max %.4f\n", label,
                           sig ? "step_signature" : "step_census", K, wrap ? "wrap" : "ghost", dead ? "dead" : "torus",
                           (long long)rows, (long long)st.waves, (int)bpc, us[us.size() / 2], us.front(), us.back());
                    fflush(stdout);
                }
    return 0;
} catch (const std::exception& e) {
    fprintf(stderr, "kbench_generic: %s\n", e.what());
    return 1;
}
