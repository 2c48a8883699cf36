// tools/sanitize_host_build.sh: BoundingVolumesHierarchy::RebuildMorton (include/gpuart_build.h on the host tree) under AddressSanitizer +
// UBSan: a triangle soup with many tied keys and one large disc, odd and even counts, down to one primitive; the rebuild with the order
// it returned itself must give the same quads, a rebuild of the rebuilt tree must be the identity, and a spoilt order must be refused.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>
#include "bvh.h"
#include "core.h"
using namespace gpuart;
int main() {
    int bad = 0;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)257, (size_t)20001}) {
        std::mt19937 rng(11);
        std::uniform_real_distribution<float> U(-10, 10), D(-0.2f, 0.2f);
        std::vector<Primitive *> prims;
        for (size_t i = 0; i + 1 < n; i++) {
            Vec3f a(U(rng), U(rng), U(rng));
            if (i % 3 == 0) a = Vec3f(std::floor(a.x), std::floor(a.y), 1.0f);   // tied keys
            prims.push_back(new Triangle(a, Vec3f(a.x + D(rng), a.y + D(rng), a.z + D(rng)), Vec3f(a.x + D(rng), a.y + D(rng), a.z + D(rng))));
        }
        prims.push_back(new Disc(Vec3f(0, 0, 0), Vec3f(0, 0, 1), 12.0f));
        BoundingVolumesHierarchy t(prims, 1024, 2), u(prims, 1024, 2);
        for (auto *p : prims) delete p;
        std::vector<uint32_t> order, again, third;
        Primitive::Data a, b, c;
        const bool ok = t.RebuildMorton(&order) && u.RebuildMorton(&again, order.data());
        t.Compile(a); u.Compile(b);
        const bool idem = t.RebuildMorton(&third);
        t.Compile(c);
        std::vector<uint32_t> iota(n);
        std::iota(iota.begin(), iota.end(), 0u);
        bool refused = true;
        if (n > 1) {
            std::vector<uint32_t> spoilt(iota);
            spoilt[0] = spoilt[1];
            refused = !t.RebuildMorton(nullptr, spoilt.data());
        }
        const bool good = ok && idem && a == b && a == c && order == again && third == iota && refused && order.size() == n;
        printf("%zu primitives: %zu floats, %s\n", n, a.size(), good ? "ok" : "WRONG");
        bad += !good;
    }
    return bad;
}
