/* temporal_fail.c — a stand-in for one entry point of libgpuart_temporal.so, for tests/test_antilag.py alone: built by the test as a shared
 * library and loaded with RTLD_GLOBAL by a child process BEFORE libgpuart.so, so that the Renderer's calls of gpuart_temporal_accumulate
 * bind here (a library loaded later looks symbols up in the global scope first). Every call goes on to the real library, named by the
 * environment variable GPUART_TEMPORAL_REAL, except the n-th committing call after temporal_fail_after(n): that one returns an error
 * without doing anything, as a device failure would. The product libraries carry no hook for this. */
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef int (*accumulate_fn)(void *, const float *, uint32_t, const void *, const int32_t *, uint32_t, uint32_t, const void *, const void *, int,
                             float *, float *);

static int countdown = 0; /* 0: no call fails */
static int failed = 0, passed_on = 0;

void temporal_fail_after(int n) { countdown = n; }
int temporal_fail_failed(void) { return failed; }
int temporal_fail_passed_on(void) { return passed_on; }

int gpuart_temporal_accumulate(void *t, const float *rgba, uint32_t spp, const void *hits, const int32_t *prims, uint32_t w, uint32_t h,
                               const void *view, const void *p, int commit, float *out_rgba, float *out_len) {
    static accumulate_fn real = NULL;
    if (!real) {
        const char *path = getenv("GPUART_TEMPORAL_REAL");
        void *lib = path ? dlopen(path, RTLD_NOW | RTLD_LOCAL) : NULL;
        real = lib ? (accumulate_fn)dlsym(lib, "gpuart_temporal_accumulate") : NULL;
        if (!real) {
            fprintf(stderr, "temporal_fail: no gpuart_temporal_accumulate in GPUART_TEMPORAL_REAL\n");
            abort();
        }
    }
    if (commit && countdown > 0 && --countdown == 0) {
        failed++;
        return -2; /* GPUART_HIP_ERR_DEVICE */
    }
    passed_on++;
    return real(t, rgba, spp, hits, prims, w, h, view, p, commit, out_rgba, out_len);
}
