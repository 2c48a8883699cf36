// trav_stack_check.cpp — gpuart_amd/csrc/hip/trav_stack.h on the CPU: is a push followed by its pop the identity on TravStack?
// trav_packet enters the upper child of an upper-only step from registers instead of pushing the entry and popping it at once
// (device_scene.h); that is exact if the pair leaves behind what it found. The very source the kernels compile, one lane, the LDS ring and
// the spill column as plain arrays. For every depth d in 0 .. 40 (the ring holds GD_RING = 8; 7, 8 and 9 are its edge): build a stack of d
// entries, apply push + pop, then compare with an untouched twin —
//   the popped entry is the pushed one; sp is what it was; every entry that is still stacked comes back, in order, from both stacks;
//   at the ring's edge the two stacks differ in `base` and in where the oldest ring entry lives, and in nothing a pop can see.
// Prints one line per depth and "identity holds at every depth"; exit code 1 on the first difference.
//   g++ -O2 -I gpuart_amd/csrc/hip -o trav_stack_check tools/trav_stack_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// the vocabulary trav_stack.h expects of its includer
#define GD_FN inline
#define GD_STACK_EVENT(writer, k)
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#define __builtin_amdgcn_wave_barrier() ((void)0)
#include "trav_stack.h"

struct Lane {  // one lane's stack: ring_stride = spill_stride = 1
    std::vector<uint2> ring_a;
    std::vector<float> ring_b;
    std::vector<uint4> spill;
    TravStack st;
    Lane() : ring_a(GD_RING), ring_b(GD_RING), spill(1024) {
        st.ring_a = ring_a.data(); st.ring_b = ring_b.data(); st.spill = spill.data();
        st.ring_stride = 1; st.spill_stride = 1;
        st.reset();
    }
};

static StackEntry entry(uint32_t k) { return StackEntry{0x1000u + k, 0.5f * (float)k, 0.25f + (float)k}; }
static bool same(const StackEntry &a, const StackEntry &b) { return a.ref == b.ref && __float_as_uint(a.pe) == __float_as_uint(b.pe) && __float_as_uint(a.he) == __float_as_uint(b.he); }

int main() {
    for (uint32_t depth = 0; depth <= 40; depth++) {
        Lane a, b;
        for (uint32_t k = 0; k < depth; k++) { a.st.push(entry(k)); b.st.push(entry(k)); }
        const uint32_t sp0 = a.st.sp, base0 = a.st.base;
        const StackEntry pushed{0xABCDEFu, -3.5f, 7.25f};
        a.st.push(pushed);
        const StackEntry popped = a.st.pop();
        if (!same(popped, pushed)) { fprintf(stderr, "depth %u: the pop did not return the entry pushed\n", depth); return 1; }
        if (a.st.sp != sp0) { fprintf(stderr, "depth %u: sp %u -> %u\n", depth, sp0, a.st.sp); return 1; }
        const bool edge = sp0 - base0 == GD_RING;  // the push spilled the oldest ring entry: base moved up by one and stays there
        if (a.st.base != base0 + (edge ? 1u : 0u)) { fprintf(stderr, "depth %u: base %u -> %u\n", depth, base0, a.st.base); return 1; }
        printf("depth %2u: sp %2u, base %2u -> %2u%s\n", depth, sp0, base0, a.st.base, edge ? "  (ring full: the oldest ring entry went to the spill column; a later pop reloads it)" : "");
        // more pushes and pops on both, then everything comes back in order
        for (uint32_t k = 0; k < 3; k++) { a.st.push(entry(100 + k)); b.st.push(entry(100 + k)); }
        for (uint32_t k = depth + 3; k-- > 0;) {
            const StackEntry ea = a.st.pop(), eb = b.st.pop();
            const StackEntry want = k >= depth ? entry(100 + k - depth) : entry(k);
            if (!same(ea, eb) || !same(ea, want)) { fprintf(stderr, "depth %u: entry %u differs after the push + pop pair\n", depth, k); return 1; }
        }
        if (a.st.sp != 0 || b.st.sp != 0 || a.st.base != 0 || b.st.base != 0) { fprintf(stderr, "depth %u: stacks not empty at the end\n", depth); return 1; }
    }
    printf("identity holds at every depth\n");
    return 0;
}
