// far_quadrupole_cpp_check.cpp -- the far-order argument of the C++ layer (host/leaf_pairs_hip.h), driven by
// tests/test_gpu_far_quadrupole.py (the arguments follow octree_cpp_check.cpp):
//   far_quadrupole_cpp_check <D> <bodies.f64> <n> <depth> <theta> <out>
// writes the forces of barnes_hut_hip_n_body<D>(bodies, theta, depth, NBX_FAR_QUADRUPOLE) as raw doubles; the test compares them with
// the Python octree plan's forces at the same order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "leaf_pairs_hip.h"
#include "nbody_hip.h"

template <int D>
static int run(char** argv) {
    const std::size_t n = (std::size_t)std::atoll(argv[3]);
    const int depth = std::atoi(argv[4]);
    const double theta = std::atof(argv[5]);
    std::vector<Body<D>> bodies(n);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || (n && std::fread(bodies.data(), sizeof(Body<D>), n, f) != n)) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::fclose(f);
    const std::vector<Vector<D>> forces = barnes_hut_hip_n_body<D>(bodies, theta, depth, NBX_FAR_QUADRUPOLE);
    FILE* o = std::fopen(argv[6], "wb");
    const bool ok = o && (forces.empty() || std::fwrite(forces.data(), sizeof(Vector<D>), forces.size(), o) == forces.size());
    if (!o || std::fclose(o) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 3; }
    std::printf("ok %zu bodies\n", n);
    return 0;
}

int main(int argc, char** argv) {
    const int D = argc == 7 ? std::atoi(argv[1]) : 0;
    if (D != 2 && D != 3) { std::fprintf(stderr, "usage: %s D bodies.f64 n depth theta out\n", argv[0]); return 1; }
    try {
        return D == 2 ? run<2>(argv) : run<3>(argv);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
}
