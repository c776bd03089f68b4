// adaptive_octree_cpp_check.cpp -- the C++ layer of the adaptive octree built on the device (host/leaf_pairs_hip.h), driven by
// tests/test_gpu_octree_adaptive.py (the arguments follow octree_cpp_check.cpp):
//   adaptive_octree_cpp_check <D> <bodies.f64> <n> <max_depth> <leaf_capacity> <theta> <out>                                       forces
//   adaptive_octree_cpp_check <D> <bodies.f64> <n> <max_depth> <leaf_capacity> <theta> <out> steps <dt> <nsteps> <rebuild_every>   bodies
// writes the forces of barnes_hut_hip_adaptive_n_body<D> as raw doubles, or the bodies barnes_hut_hip_adaptive_steps<D> leaves as raw
// Body<D> records.
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
    const int max_depth = std::atoi(argv[4]), cap = std::atoi(argv[5]);
    const double theta = std::atof(argv[6]);
    std::vector<Body<D>> bodies(n);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || (n && std::fread(bodies.data(), sizeof(Body<D>), n, f) != n)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::fclose(f);
    bool ok;
    if (argc == 12 && std::strcmp(argv[8], "steps") == 0) {
        barnes_hut_hip_adaptive_steps<D>(bodies, theta, cap, max_depth, std::atof(argv[9]), std::atoi(argv[10]), std::atoi(argv[11]));
        ok = dump(argv[7], bodies);
    } else if (argc == 8) {
        ok = dump(argv[7], barnes_hut_hip_adaptive_n_body<D>(bodies, theta, cap, max_depth));
    } else {
        return 1;
    }
    if (!ok) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 3; }
    std::printf("ok %zu bodies, capacity %d, max depth %d\n", n, cap, max_depth);
    return 0;
}

int main(int argc, char** argv) {
    const int D = argc >= 8 ? std::atoi(argv[1]) : 0;
    if (D != 2 && D != 3) { std::fprintf(stderr, "usage: %s D bodies.f64 n max_depth leaf_capacity theta out [steps dt nsteps rebuild_every]\n", argv[0]); return 1; }
    try {
        return D == 2 ? run<2>(argc, argv) : run<3>(argc, argv);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
}
