// leaf_far_cpp_check.cpp -- the C++ layer of a plan's far field (host/leaf_pairs_hip.h), driven by tests/test_gpu_far_field.py:
//   leaf_far_cpp_check <D> <bodies.f64> <n> <depth> <theta> <G> <out prefix> [no-device]
// builds build_octree_cells<D>, writes its eight arrays (<prefix>.<name>.u32) and -- unless "no-device" -- the forces of
// LeafPairSimulationHip<D> with the cells (<prefix>.forces.f64) and after removing nothing else; the test compares both with the Python path.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "leaf_pairs_hip.h"

template <class T>
static bool dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

template <int D>
static int run(const char* bodies_path, std::size_t n, int depth, double theta, double G, const std::string& prefix, bool device) {
    std::vector<Body<D>> bodies(n);
    FILE* f = std::fopen(bodies_path, "rb");
    if (!f || (n && std::fread(bodies.data(), sizeof(Body<D>), n, f) != n)) { std::fprintf(stderr, "cannot read %s\n", bodies_path); return 2; }
    std::fclose(f);
    const LeafLists L = build_octree_cells<D>(bodies, depth, theta);
    bool ok = dump(prefix + ".leaf_offsets.u32", L.leaf_offsets) && dump(prefix + ".leaf_bodies.u32", L.leaf_bodies) &&
              dump(prefix + ".list_offsets.u32", L.list_offsets) && dump(prefix + ".list_sources.u32", L.list_sources) &&
              dump(prefix + ".cell_first_leaf.u32", L.cell_first_leaf) && dump(prefix + ".cell_leaf_count.u32", L.cell_leaf_count) &&
              dump(prefix + ".far_offsets.u32", L.far_offsets) && dump(prefix + ".far_cells.u32", L.far_cells);
    if (ok && device) {
        LeafPairSimulationHip<D> sim(bodies, L);
        const std::vector<Vector<D>> forces = sim.forces(LeafLaw::TreeLeaf, G);
        ok = dump(prefix + ".forces.f64", forces);
    }
    if (!ok) { std::fprintf(stderr, "cannot write %s.*\n", prefix.c_str()); return 3; }
    std::printf("ok %zu leaves %zu cells %zu far entries\n", L.leaves(), L.cells(), L.far_cells.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: %s D bodies.f64 n depth theta G prefix [no-device]\n", argv[0]); return 1; }
    const int D = std::atoi(argv[1]);
    const std::size_t n = (std::size_t)std::atoll(argv[3]);
    const bool device = argc < 9;
    try {
        return D == 2 ? run<2>(argv[2], n, std::atoi(argv[4]), std::atof(argv[5]), std::atof(argv[6]), argv[7], device)
                      : run<3>(argv[2], n, std::atoi(argv[4]), std::atof(argv[5]), std::atof(argv[6]), argv[7], device);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
}
