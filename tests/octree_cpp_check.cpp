// octree_cpp_check.cpp -- the C++ layer of the octree built on the device (host/leaf_pairs_hip.h), driven by
// tests/test_gpu_octree_device.py (the arguments follow leaf_far_cpp_check.cpp):
//   octree_cpp_check <D> <bodies.f64> <n> <depth> <theta> <out>                                       forces
//   octree_cpp_check <D> <bodies.f64> <n> <depth> <theta> <out> steps <dt> <nsteps> <rebuild_every>   bodies after the steps
// writes the forces of barnes_hut_hip_n_body<D> as raw doubles, or the bodies barnes_hut_hip_steps<D> leaves as raw Body<D>
// records; the test compares them with the Python octree plan's forces and with LeafPlan.step_octree's bodies.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "leaf_pairs_hip.h"

template <class T>
static bool dump(const char* path, const std::vector<T>& v) {
    FILE* o = std::fopen(path, "wb");
    if (!o) return false;
    const bool ok = v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), o) == v.size();
    return std::fclose(o) == 0 && ok;
}

template <int D>
static int run(int argc, char** argv) {
    const std::size_t n = (std::size_t)std::atoll(argv[3]);
    const int depth = std::atoi(argv[4]);
    const double theta = std::atof(argv[5]);
    std::vector<Body<D>> bodies(n);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || (n && std::fread(bodies.data(), sizeof(Body<D>), n, f) != n)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::fclose(f);
    bool ok;
    if (argc >= 11 && std::strcmp(argv[7], "steps") == 0) {
        barnes_hut_hip_steps<D>(bodies, theta, depth, std::atof(argv[8]), std::atoi(argv[9]), std::atoi(argv[10]));
        ok = dump(argv[6], bodies);
    } else if (argc == 7) {
        ok = dump(argv[6], barnes_hut_hip_n_body<D>(bodies, theta, depth));
    } else {
        return 1;
    }
    if (!ok) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 3; }
    std::printf("ok %zu bodies, depth %d\n", n, depth > 0 ? depth : barnes_hut_hip_depth(n, D));
    return 0;
}

int main(int argc, char** argv) {
    const int D = argc >= 7 ? std::atoi(argv[1]) : 0;
    if (D != 2 && D != 3) { std::fprintf(stderr, "usage: %s D bodies.f64 n depth theta out [steps dt nsteps rebuild_every]\n", argv[0]); return 1; }
    try {
        return D == 2 ? run<2>(argc, argv) : run<3>(argc, argv);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
}
