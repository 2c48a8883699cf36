// bvh.h — AABB bounding-volume hierarchy of the Renderer/Scene API.
// Public surface as in the reference (src/bvh.h:46-93): construct from a primitive list with
// (maxNumLevels, minPrimitivesPerNode), Compile() into the canonical RGBA32F quad array, Print().
// Internals are different: the tree is a flat pre-order node vector that already owns the
// serialised leaf payloads, so nothing dangles after the caller deletes its primitives.
#ifndef GPUART_BVH_H
#define GPUART_BVH_H

#include <atomic>
#include <cstdint>
#include <iosfwd>
#include <memory>
#include <vector>

#include "core.h"

namespace gpuart {

struct SortKey;

class BoundingVolumesHierarchy {
public:
    // Node flags of the compiled format (reference src/bvh.h:48-52)
    static const uint32_t LEAF = 1u << 31;
    static const uint32_t IS_LOWER = 1u << 30;
    static const uint32_t IS_ROOT = 1u << 29;
    static const uint32_t FLAGS_MASK = LEAF | IS_LOWER | IS_ROOT;

    BoundingVolumesHierarchy() = default;
    BoundingVolumesHierarchy(const BoundingVolumesHierarchy &) = delete;
    BoundingVolumesHierarchy &operator=(const BoundingVolumesHierarchy &) = delete;
    BoundingVolumesHierarchy(BoundingVolumesHierarchy &&) = default;
    BoundingVolumesHierarchy &operator=(BoundingVolumesHierarchy &&) = default;

    /// Builds the tree. The order of elements in `primitives` may change.
    BoundingVolumesHierarchy(std::vector<Primitive *> &primitives, unsigned maxNumLevels, unsigned minPrimitivesPerNode);

    /// Appends the compiled tree to `compiledTree`:
    ///   node      = {xmin,ymin,zmin,pad}{xmax,ymax,zmax,pad}{flags|count, lo, hi, parent}   (uint bits in floats,
    ///               addresses in quads; the lower child follows its parent; leaves have lo = hi = 0.0f)
    ///   leaf data = per primitive {type,pad,pad,pad} + payload (Primitive::StoreIntoBVH)
    void Compile(Primitive::Data &compiledTree) const;
    /// The same quads without the vector (whose resize zeroes 105 MB on one thread for an 871 200-triangle mesh before the threads
    /// that fill it get to touch it): how many floats the compiled tree takes, and the tree written to `dst` (that many floats,
    /// uninitialised memory is fine; `baseQuad` = the quad address the tree starts at, 0 for a tree on its own).
    size_t CompiledFloats() const;
    void CompileTo(float *dst, size_t baseQuad = 0) const;

    /// Replaces primitives and refits every box; the topology stays (include/gpuart_refit.h states the contract; this is its statement on
    /// the host tree, tests/refit_ref.py the restatement). `indices`: n strictly ascending indices into the vector the constructor left
    /// behind (= the device's primitive ordinals); `payloads`: n x 16 floats, each primitive's data quads as StoreDataIntoBVH writes them,
    /// zero-padded. A primitive keeps its type. Every leaf's box becomes the running minimum / maximum of its primitives' boxes in leaf
    /// order (from +-99e29, `<` and `>`, as PrepareNode), every interior node's its lower child's box folded with its upper child's.
    /// False, with nothing changed, unless the indices are ascending and in range and every payload meets csrc/hip/prim_rule.h; if
    /// `firstBad` is given it receives the index into the list of the first offending update. n = 0 refits only.
    /// `touchedOnly`: only the leaves of the listed primitives and their ancestors are recomputed. That is the same tree wherever the
    /// rule already reproduces every box, as it does on every built and every refitted tree (a running minimum that keeps the first
    /// of equal values gives the same value folded in one pass or child by child; tests/test_refit_ref.py holds both forms to the
    /// restatement) — Renderer::UpdatePrimitives' form: a moved primitive costs its path to the root, not the whole tree.
    bool Refit(const uint32_t *indices, const float *payloads, size_t n, size_t *firstBad = nullptr, bool touchedOnly = false);
    /// The same from primitives (`moved[i]` must have the type primitive indices[i] has).
    bool Refit(const uint32_t *indices, const Primitive *const *moved, size_t n, size_t *firstBad = nullptr);
    /// Refit's verdict alone: would it accept this update? Changes nothing. With `types`, update i must also have type types[i] already.
    bool CheckRefit(const uint32_t *indices, const float *payloads, size_t n, size_t *firstBad = nullptr, const uint32_t *types = nullptr) const;
    /// The tree of a canonical compiled quad array (what Compile writes), so that Compile gives the same quads in every word the
    /// device reads. False for a malformed array.
    bool Load(const float *quads, size_t nquads);
    /// The 16 floats of Refit's `payloads` for a primitive; returns its type.
    static uint32_t Payload(const Primitive &p, float out[16]);

    /// Rebuilds the topology in Morton order over the primitives as they are now: the host's statement of include/gpuart_build.h
    /// (tests/build_ref.py is the restatement; csrc/treebuild/build.hip builds the same tree on the device). 63-bit keys from every
    /// primitive's box centre in the fold of all boxes, a stable sort by key, leaves of two, the split of a leaf range behind the last
    /// leaf that shares more key (then index) bits with the first than the range's last does, boxes by the refit rule. Afterwards
    /// Compile() writes that tree and primitive ordinal p is the old newToOld[p]. With `order` (the device's permutation) the sort is
    /// skipped and the order only checked, in linear time: a permutation, ascending by (key, old ordinal). False, with nothing changed,
    /// for an empty tree or an order that fails the check.
    bool RebuildMorton(std::vector<uint32_t> *newToOld, const uint32_t *order = nullptr);

    /// Takes over a topology built elsewhere — the device's clustered rebuild (include/gpuart_ploc.h) — over the primitives as they are
    /// now, in linear time. `newToOld`: per new ordinal the old one; `refs`: the two child refs of each of the `nRecs` records in
    /// pre-order (csrc/hip/tree_rule.h: a record's index, or REF_LEAF | flags | the leaf's first new ordinal), lower child first; with
    /// nRecs = 0 the root is a leaf of the one or two primitives. Checked before anything changes: newToOld is a permutation; the walk
    /// from record 0 meets every record exactly once and in pre-order, no deeper than 1024 levels; the leaves' ranges tile [0, N) in the
    /// order they are met, each of one or two primitives, with the flags their primitives' types ask for. The nodes' boxes are then the
    /// Refit rule's own, so Compile() writes what tests/ploc_ref.py does. False, with nothing changed, for anything else.
    bool AdoptTopology(const uint32_t *newToOld, const uint32_t *refs, size_t nRecs);

    /// Replaces the primitive list by an edited one, in the device's order (include/gpuart_edit.h states the contract; tests/edit_ref.py
    /// restates it): the primitives that are not removed in their old order, then the added ones in the order given. `remove`: nRemove
    /// strictly ascending ordinals; `addTypes`, `addPayloads`: nAdd types 0..3 and nAdd x 16 floats as for Refit. The tree is left as
    /// one leaf of all the primitives, to be rebuilt by RebuildMorton or AdoptTopology before anything is compiled from it. False,
    /// with nothing changed, unless the removals are ascending and in range, every addition meets csrc/hip/prim_rule.h and at least one
    /// primitive is left (fewer than 0x05555540); `firstBad` then receives the first offender's index, the removals counted first, or
    /// SIZE_MAX where no single entry is at fault.
    bool EditPrimitives(const uint32_t *remove, size_t nRemove, const uint32_t *addTypes, const float *addPayloads, size_t nAdd, size_t *firstBad = nullptr);
    /// The same from primitives.
    bool EditPrimitives(const uint32_t *remove, size_t nRemove, const Primitive *const *added, size_t nAdd, size_t *firstBad = nullptr);
    /// EditPrimitives' verdict alone. Changes nothing.
    bool CheckEdit(const uint32_t *remove, size_t nRemove, const uint32_t *addTypes, const float *addPayloads, size_t nAdd, size_t *firstBad = nullptr) const;

    /// Prints a compiled tree, decoding it the way the device code does.
    static void Print(const Primitive::Data &compiledTree, std::ostream &s);

    size_t GetNumNodes() const { return Nodes.size(); }
    size_t GetNumPrimitives() const { return NumPrimitives; }
    unsigned GetDepth() const { return Depth; }  ///< level of the deepest node (root = 0)

private:
    struct Node {
        float lo[3], hi[3];
        uint32_t parent;        ///< index of the parent node (root: 0)
        uint32_t higher;        ///< index of the upper child; 0 for leaves (the lower child is index+1)
        bool isLower;
        uint32_t count;         ///< primitives in a leaf (0 = interior node)
        uint32_t primFirst;     ///< leaf: position of its first primitive in the sorted primitive list
        size_t dataBegin, dataEnd;  ///< leaf payload range in LeafData (floats); filled in once the tree is complete
    };
    /// A primitive during the build: its box and itself.
    struct Item {
        float lo[3], hi[3];
        Primitive *p;
    };
    /// std::allocator whose value-less construct() leaves trivial elements uninitialised: a large buffer is then touched for the
    /// first time by the threads that fill it, not zeroed by one thread beforehand.
    template <class T>
    struct UninitAlloc : std::allocator<T> {
        template <class U> struct rebind { using other = UninitAlloc<U>; };
        template <class U> void construct(U *p) { ::new ((void *)p) U; }
        template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&...a) { ::new ((void *)p) U(std::forward<A0>(a0), std::forward<A>(a)...); }
    };
    using ItemList = std::vector<Item, UninitAlloc<Item>>;  ///< (filled by the threads that compute the boxes, not zeroed first)
    /// Sort buffers of one build task (exact_sort.h keys, the permuted primitives), grown on demand.
    struct Scratch {  // (not zeroed when they grow: every element in use is written first, by the threads that fill it)
        std::vector<SortKey, UninitAlloc<SortKey>> keys;
        ItemList items;
        void swap(Scratch &o) { keys.swap(o.keys); items.swap(o.items); }
    };
    /// A subtree under construction: nodes in pre-order with indices relative to the subtree (leaves refer to their
    /// primitives by position in the list: a subtree only ever reorders its own range of it).
    struct Subtree {
        std::vector<Node> nodes;
        unsigned depth = 0;  ///< deepest level reached (absolute)
        /// A large node built in parallel keeps only itself in `nodes`; its halves are subtrees of their own, put together
        /// once, at the end (Assemble): nothing is copied level by level.
        std::unique_ptr<Subtree> lo, hi;
        size_t base = 0;     ///< index of nodes[0] in the finished tree (Assemble)
    };
    /// Lays the pieces of a parallel build out in pre-order as `Nodes` (indices made absolute; several threads).
    void Assemble(Subtree &root, int threads);
    /// Serialises the primitives of all leaves into LeafData (Primitive::StoreIntoBVH), several threads on node ranges.
    void StoreLeaves(const ItemList &prims, int threads);
    std::vector<Node, UninitAlloc<Node>> Nodes;  ///< pre-order (every field of every node is written by Assemble's threads)
    mutable std::vector<uint32_t, UninitAlloc<uint32_t>> QuadAddr;  ///< quad address of every node relative to the tree's first quad (CompiledFloats)
    std::vector<float, UninitAlloc<float>> LeafData;  ///< serialised primitives of all leaves, in leaf order
    size_t NumPrimitives = 0;
    unsigned Depth = 0;
    /// Where primitive `index` lies: its leaf and the offset of its header quad in LeafData (floats). False if out of range.
    bool Locate(uint32_t index, uint32_t &leaf, size_t &header) const;
    mutable std::vector<uint32_t> LeafOfFirst;  ///< the leaves in pre-order = ascending primFirst (made by the first Locate)
    mutable size_t LocateCursor = 0;            ///< the entry of LeafOfFirst the last Locate found
    struct Place { uint32_t leaf; size_t header; };
    /// The verdict on an update (CheckRefit's) and, if `where` is given, where each of its primitives lies.
    bool PlanRefit(const uint32_t *indices, const float *payloads, size_t n, const uint32_t *types, size_t *firstBad, std::vector<Place> *where) const;
    void RefitNode(size_t i);  ///< node i's box by the rule, from its primitives or its children's boxes
    /// Every primitive's header in LeafData, by ordinal. False for a tree whose leaves do not number their primitives in order.
    bool PrimHeaders(std::vector<size_t> &header) const;

    /// Sequential build of [from, to) appended to `out` (reference src/bvh.cpp:35-152).
    static void Subdivide(Subtree &out, ItemList &prims, size_t from, size_t to, unsigned level,
                          unsigned maxNumLevels, unsigned minPrimitivesPerNode, uint32_t parent, bool isLower, Scratch &scratch);
    /// The same tree, built in parallel: the two halves of large nodes by different threads, and the sort
    /// of a large node itself by several (exact_sort.h: libstdc++'s introsort, re-scheduled). `spareThreads` = threads
    /// that may still be started, shared by both. Byte-identical to the sequential build: every node's permutation is
    /// the one std::sort produces, the halves work on disjoint ranges of `prims`.
    static void SubdivideParallel(Subtree &out, ItemList &prims, size_t from, size_t to, unsigned level,
                                  unsigned maxNumLevels, unsigned minPrimitivesPerNode, std::atomic<int> &spareThreads);
    /// Fills node `self` of `out` with the box of [from, to); returns true if it became a leaf, else sorts the range
    /// along the split axis and returns the split position.
    static bool PrepareNode(Subtree &out, uint32_t self, ItemList &prims, size_t from, size_t to, unsigned level,
                            unsigned maxNumLevels, unsigned minPrimitivesPerNode, size_t &split, std::atomic<int> &spareThreads,
                            Scratch &scratch);
};

}  // namespace gpuart
#endif
