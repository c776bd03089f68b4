// octree_cpp_check.cpp -- the C++ layer of the octree built on the device (host/leaf_pairs_hip.h), driven by
// tests/test_gpu_octree_device.py:
//   octree_cpp_check <bodies.f64> <n> <theta> <depth> <forces out>
// writes the forces of barnes_hut_hip_n_body<3> as raw doubles; the test compares them with the Python octree plan's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "leaf_pairs_hip.h"

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: %s bodies.f64 n theta depth forces.f64\n", argv[0]); return 1; }
    const std::size_t n = (std::size_t)std::atoll(argv[2]);
    std::vector<Body<3>> bodies(n);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || (n && std::fread(bodies.data(), sizeof(Body<3>), n, f) != n)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    try {
        const std::vector<Vector<3>> forces = barnes_hut_hip_n_body<3>(bodies, std::atof(argv[3]), std::atoi(argv[4]));
        FILE* o = std::fopen(argv[5], "wb");
        if (!o || (n && std::fwrite(forces.data(), sizeof(Vector<3>), n, o) != n) || std::fclose(o) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[5]); return 3; }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    std::printf("ok %zu bodies, depth %d\n", n, std::atoi(argv[4]) > 0 ? std::atoi(argv[4]) : barnes_hut_hip_depth(n, 3));
    return 0;
}
