// adaptive_octree_check.cpp -- build_adaptive_octree_cells<D> (host/leaf_pairs_hip.h) on the CPU, driven by
// tests/test_adaptive_octree_cpu.py and built there with g++ under ASan / UBSan:
//   adaptive_octree_check <D> <bodies.f64> <n> <max_depth> <leaf_capacity> <theta> <out.u32>
// reads n raw Body<D> records and writes the eight arrays' lengths (8 words) followed by the arrays, in the order of
// leaves.adaptive_octree_cells.  Exit status 5: the builder refused its parameters (std::invalid_argument).
// Only the host builder is called, so the program is linked without the device library (unreferenced sections are dropped).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "leaf_pairs_hip.h"

template <int D>
static int run(char** argv) {
    const std::size_t n = (std::size_t)std::atoll(argv[3]);
    std::vector<Body<D>> bodies(n);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || (n && std::fread(bodies.data(), sizeof(Body<D>), n, f) != n)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::fclose(f);
    LeafLists L;
    try {
        L = build_adaptive_octree_cells<D>(bodies, std::atoi(argv[4]), std::atoi(argv[5]), std::atof(argv[6]));
    } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 5;
    }
    const std::vector<std::uint32_t>* arrays[8] = {&L.leaf_offsets, &L.leaf_bodies, &L.list_offsets, &L.list_sources,
                                                   &L.cell_first_leaf, &L.cell_leaf_count, &L.far_offsets, &L.far_cells};
    FILE* o = std::fopen(argv[7], "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 3; }
    bool ok = true;
    for (const auto* a : arrays) { const std::uint32_t len = (std::uint32_t)a->size(); ok = ok && std::fwrite(&len, 4, 1, o) == 1; }
    for (const auto* a : arrays) ok = ok && (a->empty() || std::fwrite(a->data(), 4, a->size(), o) == a->size());
    ok = std::fclose(o) == 0 && ok;
    return ok ? 0 : 3;
}

int main(int argc, char** argv) {
    const int D = argc == 8 ? std::atoi(argv[1]) : 0;
    if (D != 2 && D != 3) { std::fprintf(stderr, "usage: %s D bodies.f64 n max_depth leaf_capacity theta out.u32\n", argv[0]); return 1; }
    return D == 2 ? run<2>(argv) : run<3>(argv);
}
