// diag_host.h — the host entry points of the three diagnostic builds (diag.h): each reads, and where it says so clears, the device counters
// of its build. Included once by gpuart_hip.hip, inside its extern "C" block; hip/exports.map passes gpuart_hip_*. The product and the
// test library define none of them; the tools declare them themselves (tools/step_stats.py, quick_box_stats.py, run_timeline.py).
#ifdef GD_STEP_STATS
/// reads (and clears) k_trace's step statistics (kernels_pipeline.h): box steps, lanes in them, leaf steps, lanes in them, rounds of the
/// wide loop, lanes holding a ray in them, refill episodes; then trav_pop's trips, the phase ticks and the packet walks' steps (box steps,
/// active lanes in them, leaf steps, active lanes in them, pushes, pop trips with and without a taker, upper-only steps): 24 words
int gpuart_hip_debug_step_stats(gpuart_hip_ctx *c, unsigned long long *out) {
    if (!c || !out) return GPUART_HIP_ERR_ARG;
    static unsigned long long zero[8];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_stats), sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_step_stats), zero, sizeof(zero)));
    HIP_TRY(hipMemcpyFromSymbol(out + 8, HIP_SYMBOL(gd::g_pop_stats), 4 * sizeof(unsigned long long)));   // out: 16 words
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gd::g_pop_stats), zero, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyFromSymbol(out + 12, HIP_SYMBOL(g_phase_ticks), 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_ticks), zero, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(gd::g_packet_stats), 8 * sizeof(unsigned long long)));  // out: 24 words
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gd::g_packet_stats), zero, 8 * sizeof(unsigned long long)));
    return 0;
}
#endif
#ifdef GD_QUICK_CHECK
/// reads (and clears) the counters of the quick box answers checked against the six face tests (device_scene.h trav_step_box)
int gpuart_hip_debug_quick_stats(gpuart_hip_ctx *c, unsigned long long *out) {
    if (!c || !out) return GPUART_HIP_ERR_ARG;
    static unsigned long long zero[8];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(gd::g_quick_stats), sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gd::g_quick_stats), zero, sizeof(zero)));
    return 0;
}
#endif
#ifdef GD_RUN_TIMELINE
/// the per-wave timeline of the last k_run launch (kernel_run.h), 24 words per wave
int gpuart_hip_debug_run_timeline(gpuart_hip_ctx *c, unsigned long long *out, size_t waves) {
    if (!c || !out || waves > 8192) return GPUART_HIP_ERR_ARG;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_run_timeline), waves * 24 * sizeof(unsigned long long)));
    return 0;
}
/// reads (and clears) the traversal-stack event counters (pushes, spilling pushes, pops, reloading pops)
int gpuart_hip_debug_stack_events(gpuart_hip_ctx *c, unsigned long long *out) {
    if (!c || !out) return GPUART_HIP_ERR_ARG;
    static unsigned long long zero[4];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(gd::g_stack_events), sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(gd::g_stack_events), zero, sizeof(zero)));
    return 0;
}
/// reads (and clears) the busy-lane histogram of the k_run launches since the last call, 256 words
int gpuart_hip_debug_run_hist(gpuart_hip_ctx *c, unsigned long long *out) {
    if (!c || !out) return GPUART_HIP_ERR_ARG;
    static unsigned long long zero[256];
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_run_hist), sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_run_hist), zero, sizeof(zero)));
    return 0;
}
#endif
