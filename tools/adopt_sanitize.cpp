// tools/sanitize_adopt.sh: BoundingVolumesHierarchy::AdoptTopology (the host tree taking over the topology of the device's clustered
// rebuild, include/gpuart_ploc.h) under AddressSanitizer + UBSan. Trees of mixed primitives with one large disc, from one primitive to a
// few thousand, and of concentric spheres (a chain); the refs are read off a tree's own compiled quads, so adopting them over the
// identity order must change nothing. Then seeded mutants of the refs and of the order: each is either refused, and the tree compiles
// to what it was, or adopted, and then the compiled tree loads again, holds every primitive and has the mutant's refs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>
#include "../gpuart_amd/csrc/hip/tree_rule.h"
#include "bvh.h"
#include "core.h"
using namespace gpuart;

static uint32_t word(const Primitive::Data &q, size_t quad, int k) {
    uint32_t u;
    memcpy(&u, &q[4 * quad + k], 4);
    return u;
}

/// The two child refs of every record of a compiled tree, in pre-order; false for a tree whose leaves hold more than two primitives.
static bool refs_of(const Primitive::Data &q, std::vector<uint32_t> &refs, size_t &prims) {
    struct Todo { size_t addr; long slot; };   // slot: where this node's ref goes (-1: the root)
    std::vector<Todo> todo{{0, -1}};
    refs.clear();
    prims = 0;
    while (!todo.empty()) {
        const Todo t = todo.back();
        todo.pop_back();
        const uint32_t flags = word(q, t.addr + 2, 0);
        uint32_t ref;
        if (flags & BoundingVolumesHierarchy::LEAF) {
            const uint32_t count = flags & ~BoundingVolumesHierarchy::FLAGS_MASK;
            if (count < 1 || count > 2) return false;
            bool tris = true;
            size_t a = t.addr + 3;
            for (uint32_t k = 0; k < count; k++) {
                const uint32_t type = word(q, a, 0);
                tris = tris && type == 2;
                a += 2 + type;
            }
            ref = tree_rule::leaf_ref((uint32_t)prims, count, tris);
            prims += count;
        } else {
            ref = (uint32_t)(refs.size() / 2);
            refs.push_back(0); refs.push_back(0);
            todo.push_back(Todo{word(q, t.addr + 2, 2), (long)(2 * ref + 1)});
            todo.push_back(Todo{word(q, t.addr + 2, 1), (long)(2 * ref)});
        }
        if (t.slot >= 0) refs[(size_t)t.slot] = ref;
    }
    return true;
}

static bool load(BoundingVolumesHierarchy &t, const Primitive::Data &q) { return t.Load(q.data(), q.size() / 4); }

int main() {
    int bad = 0;
    size_t refusedAll = 0, adoptedAll = 0;
    for (int shape = 0; shape < 2; shape++)
        for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)17, (size_t)64, (size_t)257, (size_t)3001}) {
            std::mt19937 rng(11 + (unsigned)n);
            std::uniform_real_distribution<float> U(-10, 10), D(-0.2f, 0.2f);
            std::vector<Primitive *> list;
            for (size_t i = 0; i + 1 < n; i++) {
                const Vec3f a(U(rng), U(rng), U(rng));
                if (shape == 1) list.push_back(new Sphere(Vec3f(0, 0, 0), 1.0f + (float)i / 64.0f));
                else if (i % 4 == 3) list.push_back(new Sphere(a, 0.3f));
                else list.push_back(new Triangle(a, Vec3f(a.x + D(rng), a.y + D(rng), a.z + D(rng)), Vec3f(a.x + D(rng), a.y + D(rng), a.z + D(rng))));
            }
            list.push_back(new Disc(Vec3f(0, 0, 0), Vec3f(0, 0, 1), 12.0f));
            BoundingVolumesHierarchy t(list, 1024, 2);
            for (auto *p : list) delete p;
            Primitive::Data was;
            std::vector<uint32_t> refs, iota(n);
            std::iota(iota.begin(), iota.end(), 0u);
            size_t prims = 0;
            bool good = t.RebuildMorton(nullptr);   // leaves of two
            t.Compile(was);
            good = good && refs_of(was, refs, prims) && prims == n;
            {
                BoundingVolumesHierarchy u;
                Primitive::Data now;
                good = good && load(u, was) && u.AdoptTopology(iota.data(), refs.data(), refs.size() / 2);
                u.Compile(now);
                good = good && now == was;
            }
            size_t refused = 0, adopted = 0;
            for (unsigned seed = 0; seed < 300 && good; seed++) {
                std::mt19937 m(1000 * (unsigned)n + seed);
                std::vector<uint32_t> r(refs), o(iota);
                for (int edits = 1 + (int)(m() % 3); edits > 0; edits--) {
                    std::vector<uint32_t> &v = (m() & 1) && !r.empty() ? r : o;
                    const size_t at = m() % v.size();
                    switch (m() % 5) {
                    case 0: v[at] ^= 1u << (m() % 32); break;
                    case 1: v[at] = m() % (uint32_t)(2 * n + 2); break;
                    case 2: std::swap(v[at], v[m() % v.size()]); break;
                    case 3: v[at] = m(); break;
                    default: v[at] = v[m() % v.size()]; break;
                    }
                }
                size_t recs = r.size() / 2;
                if (m() % 16 == 0 && recs) recs--;
                BoundingVolumesHierarchy u;
                Primitive::Data now;
                good = good && load(u, was);
                const bool took = u.AdoptTopology(o.data(), r.data(), recs);
                u.Compile(now);
                if (!took) {
                    refused++;
                    good = good && now == was;
                } else {
                    adopted++;
                    BoundingVolumesHierarchy w;
                    std::vector<uint32_t> back;
                    size_t held = 0;
                    good = good && load(w, now) && w.GetNumPrimitives() == n && refs_of(now, back, held) && held == n && back.size() == 2 * recs &&
                           std::equal(back.begin(), back.end(), r.begin());
                }
            }
            printf("%s, %zu primitives: %zu records, %zu mutants refused, %zu adopted, %s\n", shape ? "concentric" : "mixed", n, refs.size() / 2, refused, adopted,
                   good ? "ok" : "WRONG");
            bad += !good;
            refusedAll += refused; adoptedAll += adopted;
        }
    if (!refusedAll || !adoptedAll) { printf("the mutants were all refused or all adopted: WRONG\n"); bad++; }
    return bad;
}
