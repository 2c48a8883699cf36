// diag.h — the three diagnostic builds of libgpuart_hip.so (never the product; tools/README.md lists them and their tools):
//   -DGD_STEP_STATS    how full the steps of k_trace's waves are, trav_pop's trips, the packet walks' steps (tools/step_stats.py)
//   -DGD_QUICK_CHECK   every fast-form box test both ways, quick answer and six face tests, compared (tools/quick_box_stats.py)
//   -DGD_RUN_TIMELINE  k_run's per-wave timeline and the traversal stack's events (tools/run_timeline.py)
// A kernel states what it records in one line per site: GD_STATS(...), GD_QCHECK(...) and GD_TIMELINE(...) expand to their arguments in
// their own build and to nothing in every other one, declarations included (they stay in the scope of the site). The counters are read
// and cleared through the gpuart_hip_debug_* entry points of diag_host.h.
#pragma once
#include <hip/hip_runtime.h>

#ifdef GD_STEP_STATS
#define GD_STATS(...) __VA_ARGS__
#else
#define GD_STATS(...)
#endif
#ifdef GD_QUICK_CHECK
#define GD_QCHECK(...) __VA_ARGS__
#else
#define GD_QCHECK(...)
#endif
#ifdef GD_RUN_TIMELINE
#define GD_TIMELINE(...) __VA_ARGS__
#else
#define GD_TIMELINE(...)
#endif

namespace gd {
// trav_pop: [0] trips of its loop as waves execute them, [1] lanes in those trips, [2] calls (wave level), [3] lanes in the calls
GD_STATS(__device__ unsigned long long g_pop_stats[4];)
// trav_packet (k_trace's packets and the walking k_gen's): [0] box steps of packets, [1] active lanes in them, [2] leaf steps, [3] active lanes
// in them, [4] pushes, [5] trips of the pop loop that some lane takes, [6] trips that no lane takes, [7] upper-only steps (no lane goes down
// the lower child, some lane's walk stacks the upper one: the packet enters it from registers, no push and no pop)
GD_STATS(__device__ unsigned long long g_packet_stats[8];)
// trav_step_box: [0] boxes, [1] quick answers that stand, [2] steps, [3] steps that had to run the face tests (a lane withdrew),
// [4] standing answers that differ from the face tests (must stay 0), [5] of them: marked odd by the face tests
GD_QCHECK(__device__ unsigned long long g_quick_stats[8];)
// TravStack, counted by the lane that writes the column (GD_STACK_EVENT): pushes, pushes that spill an entry to global memory, pops, pops that reload one
GD_TIMELINE(__device__ unsigned long long g_stack_events[4];)
}  // namespace gd
#define GD_STACK_EVENT(writer, k) GD_TIMELINE(if (writer) atomicAdd(&g_stack_events[k], 1ull))

namespace {
// k_trace: box steps, lanes in them, leaf steps, lanes in them, rounds of the wide loop, lanes that hold a ray in them, refill episodes
GD_STATS(__device__ unsigned long long g_step_stats[8];)
// k_trace: summed over waves, shader-clock ticks in refill / traverse / settle + retire
GD_STATS(__device__ unsigned long long g_phase_ticks[4];)
}  // namespace
/// k_trace: the shader-clock ticks since the last mark go to `acc` (one of its ss_t_* sums)
#define GD_SS_PHASE(acc) GD_STATS({ const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - ss_mark; ss_mark = now_; })

// k_run, per wave: the 100 MHz clock at its start, when the cursor ran dry, at its end, and the lane-rounds it spent traversing (active
// lanes summed over the rounds of the TRAVERSE loop / rounds): 24 words per wave; busy lane-time and wave-time per 25 us bucket
GD_TIMELINE(__device__ unsigned long long g_run_timeline[24 * 8192];)
GD_TIMELINE(__device__ unsigned long long g_run_hist[2 * 128];)
/// k_run: one round of the TRAVERSE loop with `n` busy lanes (replicas included)
#define GD_RUN_TL_ROUND(n)                                                                                                                     \
    GD_TIMELINE({                                                                                                                              \
        tl_lanes += (unsigned long long)(n); tl_rounds++; if (exhausted) tl_tail_rounds++;                                                     \
        if (M == 2) tl_r2++; else if (M == 4) tl_r4++;                                                                                         \
        if (!exhausted) { tl_nready += n_ready; tl_nshade += n_shade; }                                                                        \
        const unsigned long long now = wall_clock64();                                                                                         \
        const unsigned bucket = (unsigned)min((now - (tl_zero ? tl_zero : tl_start)) / 2500ull, 127ull);                                       \
        if (lane_id() == 0) { tl_hist[bucket] += (unsigned)(now - tl_prev) * (unsigned)(n); tl_hist[128 + bucket] += (unsigned)(now - tl_prev); } \
        tl_prev = now;                                                                                                                         \
    })
