// converter_sanitize.cpp — csrc/hip/converter.h (host code: what stands between a caller's bytes and the device arrays of gpuart_hip_upload_bvh)
// in a stand-alone program for AddressSanitizer + UBSan and for ThreadSanitizer. Every input lies in a heap allocation of EXACTLY nquads
// quads, so that a read one quad past the end is a report. Three parts, the cases of tests/test_converter.py restated here:
//   1. the table of minimal rejections, one per message of scan() (and the deepest chain it takes);
//   2. seeded one- and two-word mutants of three small trees, one in eight also cut short: each is rejected, or converts to arrays whose
//      refs and leaf counts stay inside them;
//   3. a tree whose node table has at least 8 x 16384 entries, converted on 1, 3, 8 and 64 threads: identical bytes.
// tools/sanitize_converter.sh builds and runs it both ways (CPU only).   converter_sanitize [mutants]
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>

#include "converter.h"

namespace {

const uint32_t LEAF = 1u << 31, IS_LOWER = 1u << 30, IS_ROOT = 1u << 29;

float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Prim { uint32_t type; std::vector<float> d; float lo[3], hi[3]; };

Prim sphere(float x, float y, float z, float r) {
    Prim p{P_SPHERE, {x, y, z, r}, {x - r, y - r, z - r}, {x + r, y + r, z + r}};
    return p;
}
Prim disc(float x, float y, float z, float r) {
    Prim p{P_DISC, {x, y, z, r, 0, 0, 1, 0}, {x - r, y - r, z - r}, {x + r, y + r, z + r}};
    return p;
}
Prim triangle(const float v[9]) {
    Prim p{P_TRIANGLE, {v[0], v[1], v[2], 0, v[3], v[4], v[5], 0, v[6], v[7], v[8], 0}, {}, {}};
    for (int k = 0; k < 3; k++) { p.lo[k] = std::min(v[k], std::min(v[3 + k], v[6 + k])); p.hi[k] = std::max(v[k], std::max(v[3 + k], v[6 + k])); }
    return p;
}
/// A cone along +z (the constants as the reference's constructor derives them).
Prim cone(float x, float y, float z, float len, float r1, float r2) {
    float cosb = 0;
    if (std::fabs(r1 - r2) >= 1.0e-7f) {
        const float rr = r1 > r2 ? r1 : r2, h = rr * len / std::fabs(r1 - r2);
        cosb = (r1 > r2 ? rr : -rr) / std::sqrt(h * h + rr * rr);
    }
    Prim p{P_CONE, {x, y, z, r1, x, y, z + len, r2, 0, 0, 1, len, (r2 - r1) / len, cosb, z, 0}, {}, {}};
    const float c1[3] = {x, y, z}, c2[3] = {x, y, z + len};
    for (int k = 0; k < 3; k++) { p.lo[k] = std::min(c1[k] - r1, c2[k] - r2); p.hi[k] = std::max(c1[k] + r1, c2[k] + r2); }
    return p;
}

struct Node {
    std::vector<Prim> prims;  // a leaf's
    std::unique_ptr<Node> lo, hi;
};
std::unique_ptr<Node> leaf(std::vector<Prim> p) { auto n = std::make_unique<Node>(); n->prims = std::move(p); return n; }
std::unique_ptr<Node> join(std::unique_ptr<Node> a, std::unique_ptr<Node> b) { auto n = std::make_unique<Node>(); n->lo = std::move(a); n->hi = std::move(b); return n; }

/// The reference's CompileFrom layout: node, lower subtree, upper subtree; an interior box is the union of its children's.
void emit(const Node &n, std::vector<float> &q, uint32_t parent, uint32_t flags, float bmin[3], float bmax[3]) {
    const size_t addr = q.size() / 4;
    q.insert(q.end(), 12, 0.0f);
    if (!n.lo) {
        for (int k = 0; k < 3; k++) { bmin[k] = 9.9e30f; bmax[k] = -9.9e30f; }
        for (const Prim &p : n.prims) {
            for (int k = 0; k < 3; k++) { bmin[k] = std::min(bmin[k], p.lo[k]); bmax[k] = std::max(bmax[k], p.hi[k]); }
            q.push_back(f_of(p.type)); q.insert(q.end(), 3, 0.0f);
            q.insert(q.end(), p.d.begin(), p.d.end());
        }
        q[4 * addr + 8] = f_of(LEAF | flags | (uint32_t)n.prims.size());
    } else {
        float lmin[3], lmax[3], hmin[3], hmax[3];
        emit(*n.lo, q, (uint32_t)addr, IS_LOWER, lmin, lmax);
        const size_t hi = q.size() / 4;
        emit(*n.hi, q, (uint32_t)addr, 0, hmin, hmax);
        for (int k = 0; k < 3; k++) { bmin[k] = std::min(lmin[k], hmin[k]); bmax[k] = std::max(lmax[k], hmax[k]); }
        q[4 * addr + 8] = f_of(flags); q[4 * addr + 9] = f_of((uint32_t)addr + 3); q[4 * addr + 10] = f_of((uint32_t)hi);
    }
    q[4 * addr + 11] = f_of(parent);
    for (int k = 0; k < 3; k++) { q[4 * addr + k] = bmin[k]; q[4 * addr + 4 + k] = bmax[k]; }
}
std::vector<float> compile(const Node &n) {
    std::vector<float> q;
    float a[3], b[3];
    emit(n, q, 0, IS_ROOT, a, b);
    return q;
}

const float T1[9] = {0, 0, 0.5f, 1, 0, 0.25f, 0, 1, 0.75f}, T2[9] = {-1, 0.5f, 0.25f, -0.5f, 1, 0.5f, -0.75f, 0.25f, 1},
            T3[9] = {0.5f, 0.5f, 0.5f, 0.75f, 0.5f, 0.5f, 0.5f, 0.75f, 1};
Prim SPH() { return sphere(0.25f, 0.5f, 0.75f, 0.125f); }

/// `levels` interior nodes, each with a one-sphere leaf below and the next link above.
std::vector<float> chain(unsigned levels) {
    std::vector<float> piece = compile(*leaf({SPH()}));
    std::vector<float> q((size_t)(8 * levels + 5) * 4, 0.0f);
    for (unsigned i = 0; i <= levels; i++) {
        const size_t a = 8 * (size_t)i;
        if (i < levels) {
            memcpy(&q[4 * a], piece.data(), 32);
            q[4 * a + 8] = f_of(i ? 0u : IS_ROOT); q[4 * a + 9] = f_of((uint32_t)a + 3); q[4 * a + 10] = f_of((uint32_t)a + 8);
            memcpy(&q[4 * (a + 3)], piece.data(), piece.size() * 4);
            q[4 * (a + 5)] = f_of(LEAF | IS_LOWER | 1u);
        } else {
            memcpy(&q[4 * a], piece.data(), piece.size() * 4);
            q[4 * (a + 2)] = f_of(LEAF | 1u);
        }
    }
    return q;
}

int failures = 0;
void expect(bool ok, const char *what, const std::string &detail = "") {
    if (!ok) { failures++; printf("FAILED: %s %s\n", what, detail.c_str()); }
}

struct Result {
    std::string err;
    std::vector<float4, UninitAlloc<float4>> recs, prims;
    uint32_t root_ref = 0;
};

/// Converts the first nq quads of `q` from an allocation of exactly that size.
Result run(const std::vector<float> &q, size_t nq, unsigned threads, uint32_t top_depth = 0) {
    float *exact = (float *)malloc(nq * 16);
    memcpy(exact, q.data(), nq * 16);
    Result r;
    {
        Converter cv;
        cv.q = exact; cv.nq = nq; cv.top_depth = top_depth;
        Converter::Child root;
        if (!cv.convert(root, threads)) r.err = cv.err;
        else { r.recs.swap(cv.recs); r.prims.swap(cv.prims); r.root_ref = root.ref; }
    }
    free(exact);
    return r;
}

/// What the kernels rely on: interior refs inside recs, a leaf's primitives inside prims, the ref's flag bits true of them.
bool device_safe(const Result &r) {
    const size_t n_recs = r.recs.size() / 4, n_prims = r.prims.size() / 3;
    std::vector<uint32_t> refs{r.root_ref};
    for (size_t k = 0; k < n_recs; k++) { refs.push_back(u_of(r.recs[4 * k].w)); refs.push_back(u_of(r.recs[4 * k + 1].w)); }
    for (uint32_t x : refs) {
        if (!(x & GD_REF_LEAF)) { if (x >= n_recs) return false; continue; }
        const size_t first = x & GD_REF_INDEX;
        if (first >= n_prims) return false;
        const uint32_t count = u_of(r.prims[3 * first].w) >> 2;
        if (first + std::max<size_t>(count, 1) > n_prims) return false;
        bool tris = count == 1 || count == 2;
        for (uint32_t k = 0; k < count; k++) {
            const uint32_t T = u_of(r.prims[3 * (first + k)].w);
            if (k && T > 3) return false;
            if ((T & 3) != P_TRIANGLE) tris = false;
        }
        const bool small = (count == 1 || count == 2) && !tris;
        if (!!(x & GD_REF_TRIS) != tris || !!(x & GD_REF_SMALL) != small || !!(x & GD_REF_TWO) != (count == 2)) return false;
    }
    return true;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {  // xorshift64*, fixed seed: the same mutants every run
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

std::unique_ptr<Node> balanced(size_t from, size_t to) {
    if (to - from == 1) {
        const float x = (float)(from % 256) / 128.0f - 1.0f, y = (float)(from / 256 % 256) / 128.0f - 1.0f, z = (float)(from / 65536) * 0.25f + 0.5f;
        switch (from % 4) {
        case 0: return leaf({sphere(x, y, z, 0.003f)});
        case 1: { const float v[9] = {x, y, z, x + 0.004f, y, z, x, y + 0.004f, z + 0.002f}; return leaf({triangle(v), triangle(v)}); }
        case 2: return leaf({disc(x, y, z, 0.003f), sphere(x, y, z, 0.002f)});
        default: return leaf({cone(x, y, z, 0.01f, 0.003f, 0.001f)});
        }
    }
    const size_t mid = from + (to - from + 1) / 2;
    return join(balanced(from, mid), balanced(mid, to));
}

}  // namespace

int main(int argc, char **argv) {
    const unsigned n_mutants = argc > 1 ? (unsigned)atoi(argv[1]) : 200000u;
    std::vector<Prim> tt;
    tt.push_back(triangle(T1)); tt.push_back(triangle(T2));
    std::vector<Prim> root_prims; root_prims.push_back(SPH()); root_prims.push_back(triangle(T1)); root_prims.push_back(disc(0.5f, -0.25f, 0.25f, 0.375f));
    std::vector<Prim> st; st.push_back(SPH()); st.push_back(triangle(T1));
    std::vector<Prim> ds; ds.push_back(disc(0.5f, -0.25f, 0.25f, 0.375f)); ds.push_back(sphere(-0.5f, 0.25f, 0.5f, 0.25f));
    std::vector<Prim> t3; t3.push_back(triangle(T1)); t3.push_back(triangle(T2)); t3.push_back(triangle(T3));
    const std::vector<float> root_leaf = compile(*leaf(root_prims));
    const std::vector<float> two = compile(*join(leaf({SPH()}), leaf(tt)));
    const std::vector<float> mixed = compile(*join(join(leaf(st), join(leaf({cone(0.5f, -0.75f, 0, 0.375f, 0.25f, 0.125f)}), leaf(ds))),
                                                   join(leaf(t3), leaf({triangle(T3)}))));
    expect(two.size() == 19 * 4, "the two-leaf tree has 19 quads");
    for (const auto *t : {&root_leaf, &two, &mixed}) {
        for (unsigned threads : {1u, 8u}) {
            Result r = run(*t, t->size() / 4, threads, 2);
            expect(r.err.empty() && device_safe(r), "a small tree converts", r.err);
        }
    }

    // 1. one minimal mutation per message
    {
        auto edit = [&](size_t quad, int word, uint32_t v) { std::vector<float> t = two; t[4 * quad + word] = f_of(v); return t; };
        struct Case { const char *name; std::vector<float> q; size_t nq; const char *message; };
        const std::vector<float> deep = chain(1025), deepest = chain(1024);
        const Case table[] = {
            {"root cut off", two, 2, "node address out of range"},
            {"chain of 1025 levels", deep, deep.size() / 4, "tree deeper than 1024 levels"},
            {"a count of three in a leaf of two", edit(10, 0, LEAF | 3), 19, "primitive header out of range"},
            {"type 4", edit(11, 0, 4), 19, "unknown primitive type"},
            {"last data quad cut off", two, 18, "primitive data out of range"},
            {"lower child one quad late", edit(2, 1, 4), 19, "lower child does not follow its parent"},
            {"upper child at nquads", edit(2, 2, 19), 19, "upper child address out of range"},
            {"upper child not above the lower", edit(2, 2, 3), 19, "upper child address out of range"},
            {"upper child one quad late", edit(2, 2, 9), 19, "upper child does not start where the lower subtree ends"},
            {"upper child inside the lower subtree", edit(2, 2, 5), 19, "upper child does not start where the lower subtree ends"},
        };
        for (const Case &c : table) {
            Result r = run(c.q, c.nq, 1);
            expect(r.err == c.message, c.name, "-> '" + r.err + "'");
        }
        Result r = run(deepest, deepest.size() / 4, 1);
        expect(r.err.empty() && device_safe(r), "chain of 1024 levels", r.err);
        printf("rejections: %zu cases\n", sizeof table / sizeof table[0]);
    }

    // 2. mutants
    {
        const std::vector<float> *trees[3] = {&root_leaf, &two, &mixed};
        std::map<std::string, unsigned> seen;
        unsigned accepted = 0;
        for (unsigned i = 0; i < n_mutants; i++) {
            std::vector<float> t = *trees[i % 3];
            const uint32_t nq = (uint32_t)(t.size() / 4);
            for (unsigned k = 0, n = 1 + rnd(2); k < n; k++) {
                size_t word = rnd(4 * nq);                                                // any word ...
                if (rnd(2)) word = 4 * (size_t)rnd(nq) + (rnd(4) ? 0 : 1 + rnd(3));        // ... or, half of the time, mostly first words of quads (flags, types)
                const uint32_t old = u_of(t[word]);
                const uint32_t values[9] = {0u, 1u + rnd(8), nq - 1, nq, nq + 1, LEAF | rnd(6), LEAF | (rnd(2) ? 1000u : 0x1fffffffu), 0xffffffffu, old ^ (1u << rnd(32))};
                t[word] = f_of(values[rnd(9)]);
            }
            const size_t cut = rnd(8) ? nq : 1 + rnd(nq - 1);
            Result r = run(t, cut, 1 + rnd(3));
            if (r.err.empty()) { accepted++; expect(device_safe(r), "an accepted mutant stays inside its arrays", "mutant " + std::to_string(i)); }
            else seen[r.err]++;
        }
        printf("mutants: %u, accepted %u = %.1f %%\n", n_mutants, accepted, 100.0 * accepted / n_mutants);
        for (const auto &kv : seen) printf("  %7u  %s\n", kv.second, kv.first.c_str());
        expect(accepted >= n_mutants / 10 && n_mutants - accepted >= n_mutants / 10 && seen.size() == 7, "the mutant set reaches both verdicts and seven messages");
    }

    // 3. the fill pass on several threads
    {
        const std::vector<float> big = compile(*balanced(0, 70000));
        Result one = run(big, big.size() / 4, 1);
        expect(one.err.empty() && device_safe(one), "the big tree converts", one.err);
        const size_t nodes = one.recs.size() / 4 * 2 + 1;
        expect(nodes >= 8 * 16384, "the big tree's node table has at least 8 x 16384 entries");
        for (unsigned threads : {3u, 8u, 64u}) {
            Result r = run(big, big.size() / 4, threads, 4);
            Result plain = run(big, big.size() / 4, threads);
            expect(r.err.empty() && plain.err.empty() && plain.recs.size() == one.recs.size() && plain.prims.size() == one.prims.size() &&
                   !memcmp(plain.recs.data(), one.recs.data(), one.recs.size() * 16) && !memcmp(plain.prims.data(), one.prims.data(), one.prims.size() * 16) &&
                   !memcmp(r.prims.data(), one.prims.data(), one.prims.size() * 16) && plain.root_ref == one.root_ref,
                   "identical arrays on several threads", std::to_string(threads));
        }
        printf("threads: %zu nodes, %zu records, %zu primitives on 1, 3, 8, 64 threads\n", nodes, one.recs.size() / 4, one.prims.size() / 3);
    }
    printf(failures ? "converter.h: %d FAILED\n" : "converter.h: ok\n", failures);
    return failures ? 1 : 0;
}
