// trav_stack.h — the traversal stack of the BVH queries (device_scene.h includes it inside namespace gd, after diag.h). The file names
// no header of its own: GD_FN, uint2 / uint4 with their make_ functions, __float_as_uint / __uint_as_float, the two wave builtins of
// replica_fence and GD_STACK_EVENT are the includer's, so that tools/trav_stack_check.cpp can run this very source on the CPU
// (tests/test_issue_budget.py: a push followed by its pop at the ring's edge).
#pragma once

// ---- traversal stack: short per-lane ring in LDS + spill to global memory -------------------------
// Entry = (upper child's ref, parent's box-entry parameter, the child's own box-entry parameter).
// Entries [base, sp) live in the LDS ring (slot = index % RING, one column per
// lane -> conflict-free accesses); entries [0, base) live in a per-lane global spill column. The oldest
// entries (closest to the root, popped last) are the ones spilled, so spills are rare; any tree depth
// up to the reference's 1024 levels works without a separate code path.
#ifndef GD_RING
#define GD_RING 8
#endif

struct StackEntry {
    uint32_t ref;   ///< upper child: record index, or GD_REF_LEAF | first primitive
    float pe, he;   ///< box-entry parameter of the parent / of the child itself (GD_ENTRY_MISS: box not hit)
};

#if (GD_RING & (GD_RING - 1)) == 0
#define GD_RING_SLOT(i) ((i) & (GD_RING - 1))
#else
#define GD_RING_SLOT(i) ((i) % GD_RING)  // i < 1024 + GD_RING: a multiply-shift
#endif

struct TravStack {
    uint2 *ring_a;           ///< LDS, [GD_RING][BLOCK]: (ref, pe)
    float *ring_b;           ///< LDS, [GD_RING][BLOCK]: he
    uint4 *spill;            ///< global, [levels][total_lanes]; this lane's column is spill[level * spill_stride]
    uint32_t ring_stride;    ///< BLOCK
    uint32_t spill_stride;   ///< total lanes of the launch
    uint32_t sp, base;
    GD_FN void reset() { sp = 0; base = 0; }
    /// The replicas of a ray (thin-wave modes) read what its first replica stored: the stores of `if (writer)` must stay ahead
    /// of the other lanes' loads in the instruction stream. Per thread the compiler could legally turn "conditional store, then
    /// load" into "writer keeps the value, the others load" and run the others first; a wavefront-scope fence (no instruction:
    /// a wave executes its memory operations in order) plus a wave barrier pin the order.
    static GD_FN void replica_fence() {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    /// `writer`: this lane performs the stores. A ray that several lanes carry as identical replicas (the thin-wave modes
    /// below) has ONE column; every replica keeps sp / base and reads the column, only the first one writes it.
    GD_FN void push(StackEntry e, bool writer = true) {
        GD_STACK_EVENT(writer, 0);
        if (sp - base == GD_RING) {
            GD_STACK_EVENT(writer, 1);
            uint32_t o = GD_RING_SLOT(base) * ring_stride;
            uint2 a = ring_a[o];
            if (writer) spill[(size_t)base * spill_stride] = make_uint4(a.x, a.y, __float_as_uint(ring_b[o]), 0);
            replica_fence();
            base++;
        }
        uint32_t o = GD_RING_SLOT(sp) * ring_stride;
        if (writer) {
            ring_a[o] = make_uint2(e.ref, __float_as_uint(e.pe));
            ring_b[o] = e.he;
        }
        replica_fence();
        sp++;
    }
    GD_FN StackEntry pop(bool writer = true) {  // precondition: sp > 0
        GD_STACK_EVENT(writer, 2);
        if (sp == base) {
            GD_STACK_EVENT(writer, 3);
            base--;
            uint4 v = spill[(size_t)base * spill_stride];
            uint32_t o = GD_RING_SLOT(base) * ring_stride;
            if (writer) {
                ring_a[o] = make_uint2(v.x, v.y);
                ring_b[o] = __uint_as_float(v.z);
            }
            replica_fence();
        }
        sp--;
        uint32_t o = GD_RING_SLOT(sp) * ring_stride;
        uint2 a = ring_a[o];
        StackEntry e;
        e.ref = a.x; e.pe = __uint_as_float(a.y); e.he = ring_b[o];
        // Keep the entry's three words in the two LDS reads issued here: left alone the compiler reads the parameters first (4 + 4 bytes),
        // compares, and fetches the ref with a THIRD read once the entry is accepted — a second LDS round trip in the dependent chain
        // pop -> enter -> record address -> fetch of every step that ends in a pop.
#ifdef __HIP_DEVICE_COMPILE__  // (the CPU check has no vector registers to name)
        asm volatile("" : "+v"(e.ref), "+v"(e.pe), "+v"(e.he));
#endif
        return e;
    }
};
