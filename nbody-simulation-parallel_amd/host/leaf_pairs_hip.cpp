// leaf_pairs_hip.cpp -- C++ shim of the leaf-pair direct sums onto the C ABI + the uniform leaf builder.
#include "leaf_pairs_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <stdexcept>
#include <string>
#include <unordered_map>

#include "nbody_hip.h"
#include "../csrc/octree_device.h"   // its plain C++ part: root_box, body_key, packed_coords, accepts_box (one definition, host and device)

namespace {
thread_local float g_leaf_ms = 0.0f;
}

float last_leaf_pair_kernel_ms() { return g_leaf_ms; }

template <int D>
std::vector<Vector<D>> leaf_pair_direct_forces_hip(const std::vector<Body<D>>& bodies, const LeafLists& L, LeafLaw law) {
    if (L.leaf_offsets.empty() || L.list_offsets.size() != L.leaf_offsets.size())
        throw std::runtime_error("leaf_pair_direct_forces_hip: leaf_offsets and list_offsets need n_leaves + 1 entries");
    std::vector<Vector<D>> forces(bodies.size());
    int device = 0;
    if (const char* e = std::getenv("NBODY_HIP_DEVICE")) device = std::atoi(e);
    g_leaf_ms = 0.0f;
    const int rc = nbx_leaf_pair_forces(bodies.data(), bodies.size(), D, sizeof(Body<D>), L.leaf_offsets.data(), L.leaf_bodies.data(),
                                        L.leaves(), L.list_offsets.data(), L.list_sources.data(), static_cast<int>(law), NBX_REFERENCE_G,
                                        device, reinterpret_cast<double*>(forces.data()), &g_leaf_ms);
    if (rc != NBX_OK) {
        std::string msg = std::string("leaf_pair_direct_forces_hip: ") + nbx_strerror(rc);
        const char* detail = nbx_last_error_detail();
        if (detail && *detail) msg += std::string(" -- ") + detail;
        throw std::runtime_error(msg);
    }
    return forces;
}

namespace {
[[noreturn]] void raise_leaf(const char* where, int rc) {
    std::string msg = std::string(where) + ": " + nbx_strerror(rc);
    const char* detail = nbx_last_error_detail();
    if (detail && *detail) msg += std::string(" -- ") + detail;
    throw std::runtime_error(msg);
}
int leaf_device() {
    if (const char* e = std::getenv("NBODY_HIP_DEVICE")) return std::atoi(e);
    return 0;
}
}  // namespace

template <int D>
LeafPairSimulationHip<D>::LeafPairSimulationHip(const std::vector<Body<D>>& bodies, const LeafLists& L) : n_(bodies.size()) {
    if (L.leaf_offsets.empty() || L.list_offsets.size() != L.leaf_offsets.size())
        throw std::runtime_error("LeafPairSimulationHip: leaf_offsets and list_offsets need n_leaves + 1 entries");
    const int device = leaf_device();
    int rc = nbx_leaf_plan_create(&plan_, device, D, n_, L.leaf_offsets.data(), L.leaf_bodies.data(), L.leaves(), L.list_offsets.data(),
                                  L.list_sources.data());
    if (!rc && L.cells()) {
        if (L.cell_leaf_count.size() != L.cells() || L.far_offsets.size() != L.leaf_offsets.size()) {
            nbx_leaf_plan_destroy(plan_);
            plan_ = nullptr;
            throw std::runtime_error("LeafPairSimulationHip: cell_leaf_count needs n_cells entries and far_offsets n_leaves + 1");
        }
        rc = nbx_leaf_plan_set_cells(plan_, L.cell_first_leaf.data(), L.cell_leaf_count.data(), L.cells(), L.far_offsets.data(), L.far_cells.data());
    }
    if (!rc) rc = nbx_ctx_create(&ctx_, device, D, n_, 1, 0);
    if (!rc) rc = nbx_ctx_upload_bodies(ctx_, bodies.data(), sizeof(Body<D>));
    if (rc != NBX_OK) {
        nbx_leaf_plan_destroy(plan_);
        nbx_ctx_destroy(ctx_);
        plan_ = nullptr; ctx_ = nullptr;
        raise_leaf("LeafPairSimulationHip", rc);
    }
}
template <int D>
LeafPairSimulationHip<D>::~LeafPairSimulationHip() {
    nbx_leaf_plan_destroy(plan_);   // before the context: its last evaluation may still be queued on the context's stream
    nbx_ctx_destroy(ctx_);
}
template <int D>
std::vector<Vector<D>> LeafPairSimulationHip<D>::forces(LeafLaw law, double G) {
    std::vector<Vector<D>> f(n_);
    const int rc = nbx_leaf_plan_forces_ctx(plan_, ctx_, static_cast<int>(law), G, reinterpret_cast<double*>(f.data()), nullptr);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::forces", rc);
    return f;
}
template <int D>
void LeafPairSimulationHip<D>::evaluate(LeafLaw law, double G) {
    int rc = nbx_leaf_plan_forces_ctx(plan_, ctx_, static_cast<int>(law), G, nullptr, nullptr);
    if (!rc) rc = nbx_ctx_synchronize(ctx_);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::evaluate", rc);
}
template <int D>
void LeafPairSimulationHip<D>::step(LeafLaw law, double G, double dt, int nsteps) {
    const int rc = nbx_leaf_plan_step(plan_, ctx_, static_cast<int>(law), G, dt, nsteps);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::step", rc);
}
template <int D>
void LeafPairSimulationHip<D>::step_kdk(LeafLaw law, double G, double dt, int nsteps) {
    const int rc = nbx_leaf_plan_step_kdk(plan_, ctx_, static_cast<int>(law), G, dt, nsteps);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::step_kdk", rc);
}
template <int D>
nbx_step_clock LeafPairSimulationHip<D>::step_kdk_adaptive(LeafLaw law, double G, const nbx_step_control& control, int max_steps) {
    nbx_step_clock clock{};
    clock.t = control.t_start;
    int rc = nbx_leaf_plan_step_kdk_adaptive(plan_, ctx_, static_cast<int>(law), G, &control, max_steps, 0);
    if (!rc && max_steps > 0) rc = nbx_leaf_plan_get_step_clock(plan_, &clock);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::step_kdk_adaptive", rc);
    return clock;
}
template <int D>
void LeafPairSimulationHip<D>::synchronize() {
    const int rc = nbx_ctx_synchronize(ctx_);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::synchronize", rc);
}
template <int D>
void LeafPairSimulationHip<D>::download(std::vector<Body<D>>& bodies) {
    if (bodies.size() != n_) throw std::runtime_error("LeafPairSimulationHip::download: body count differs");
    const int rc = nbx_ctx_download_bodies(ctx_, bodies.data(), sizeof(Body<D>));
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::download", rc);
}
template <int D>
void LeafPairSimulationHip<D>::set_far_order(int order) {
    const int rc = nbx_leaf_plan_set_far_order(plan_, order);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::set_far_order", rc);
}
template <int D>
void LeafPairSimulationHip<D>::set_softening(double epsilon) {
    const int rc = nbx_leaf_plan_set_softening(plan_, epsilon);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::set_softening", rc);
}
template <int D>
float LeafPairSimulationHip<D>::single_launch_ms(LeafLaw law, double G) {
    float ms = 0.0f;
    const int rc = nbx_leaf_plan_forces_ctx(plan_, ctx_, static_cast<int>(law), G, nullptr, &ms);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::single_launch_ms", rc);
    return ms;
}
template <int D>
float LeafPairSimulationHip<D>::back_to_back_ms(LeafLaw law, int reps) {
    float ms = 0.0f;
    const int rc = nbx_leaf_plan_time_kernel(plan_, static_cast<int>(law), reps, &ms);
    if (rc != NBX_OK) raise_leaf("LeafPairSimulationHip::back_to_back_ms", rc);
    return ms;
}
template class LeafPairSimulationHip<2>;
template class LeafPairSimulationHip<3>;

int barnes_hut_hip_depth(std::size_t n_bodies, int dim) {
    int depth = 0;
    while (depth < 10 && static_cast<double>(n_bodies) / std::pow(2.0, depth * dim) > 16.0) ++depth;
    return depth;
}

namespace {
// a context holding the bodies and a plan with the octree built from them; both destroyed on every way out
template <int D>
struct OctreeOnDevice {
    nbx_ctx* ctx = nullptr;
    nbx_leaf_plan* plan = nullptr;
    // leaf_capacity < 0: the fixed-depth tree (depth 0: barnes_hut_hip_depth); otherwise the adaptive one, depth = max_depth
    OctreeOnDevice(const std::vector<Body<D>>& bodies, double theta, int depth, const char* where, int leaf_capacity = -1, int far_order = NBX_FAR_MONOPOLE) {
        const int device = leaf_device();
        int rc = nbx_ctx_create(&ctx, device, D, bodies.size(), 1, 0);
        if (!rc) rc = nbx_ctx_upload_bodies(ctx, bodies.data(), sizeof(Body<D>));
        if (!rc && leaf_capacity >= 0) rc = nbx_leaf_plan_create_octree_adaptive(&plan, ctx, depth, leaf_capacity, theta);
        else if (!rc) rc = nbx_leaf_plan_create_octree(&plan, ctx, depth > 0 ? depth : barnes_hut_hip_depth(bodies.size(), D), theta);
        if (!rc && far_order != NBX_FAR_MONOPOLE) rc = nbx_leaf_plan_set_far_order(plan, far_order);
        if (rc != NBX_OK) {
            nbx_leaf_plan_destroy(plan);
            nbx_ctx_destroy(ctx);
            raise_leaf(where, rc);
        }
    }
    ~OctreeOnDevice() {
        nbx_leaf_plan_destroy(plan);   // before the context, as in LeafPairSimulationHip
        nbx_ctx_destroy(ctx);
    }
};
}  // namespace

template <int D>
std::vector<Vector<D>> barnes_hut_hip_n_body(const std::vector<Body<D>>& bodies, double theta, int depth, int far_order) {
    std::vector<Vector<D>> forces(bodies.size());
    if (bodies.empty()) return forces;
    OctreeOnDevice<D> tree(bodies, theta, depth, "barnes_hut_hip_n_body", -1, far_order);
    const int rc = nbx_leaf_plan_forces_ctx(tree.plan, tree.ctx, static_cast<int>(LeafLaw::TreeLeaf), NBX_REFERENCE_G, reinterpret_cast<double*>(forces.data()), nullptr);
    if (rc != NBX_OK) raise_leaf("barnes_hut_hip_n_body", rc);
    return forces;
}

template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order) {
    if (bodies.empty()) return;
    OctreeOnDevice<D> tree(bodies, theta, depth, "barnes_hut_hip_steps", -1, far_order);
    int rc = nbx_leaf_plan_step_octree(tree.plan, tree.ctx, static_cast<int>(LeafLaw::TreeLeaf), NBX_REFERENCE_G, dt, nsteps, rebuild_every);
    if (!rc) rc = nbx_ctx_download_bodies(tree.ctx, bodies.data(), sizeof(Body<D>));
    if (rc != NBX_OK) raise_leaf("barnes_hut_hip_steps", rc);
}

namespace {
// the smallest and largest step of the plan's last adaptive call, from its history (the closing evaluation's entry has dt = 0)
int adaptive_step_range(nbx_leaf_plan* plan, double* dt_smallest, double* dt_largest) {
    *dt_smallest = *dt_largest = 0.0;
    std::size_t count = 0;
    int rc = nbx_leaf_plan_get_step_history(plan, nullptr, nullptr, 0, &count);
    if (rc || !count) return rc;
    std::vector<double> dt(count);
    rc = nbx_leaf_plan_get_step_history(plan, nullptr, dt.data(), count, &count);
    for (std::size_t i = 0; !rc && i < count; ++i) {
        if (dt[i] == 0.0) continue;
        *dt_smallest = *dt_smallest == 0.0 ? dt[i] : std::min(*dt_smallest, dt[i]);
        *dt_largest = std::max(*dt_largest, dt[i]);
    }
    return rc;
}

// one adaptive call and what it reports; max_steps == 0 does nothing and reports a clock standing at t_start
int adaptive_steps(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, int max_steps, int rebuild_every, TreeAdaptiveSteps* steps, const char* where) {
    if (!steps) throw std::runtime_error(std::string(where) + ": TreeIntegrator::KickDriftKickAdaptive needs its TreeAdaptiveSteps");
    steps->clock = nbx_step_clock{};
    steps->clock.t = steps->control.t_start;
    steps->dt_smallest = steps->dt_largest = 0.0;
    int rc = nbx_leaf_plan_step_kdk_adaptive(plan, ctx, law, G, &steps->control, max_steps, rebuild_every);
    if (!rc && max_steps > 0) rc = nbx_leaf_plan_get_step_clock(plan, &steps->clock);
    if (!rc && max_steps > 0) rc = adaptive_step_range(plan, &steps->dt_smallest, &steps->dt_largest);
    return rc;
}

// the reference law's step loop under any integrator, the bodies brought back at the end
template <int D>
void tree_leaf_steps(OctreeOnDevice<D>& tree, std::vector<Body<D>>& bodies, double dt, int nsteps, int rebuild_every, TreeIntegrator integrator, TreeAdaptiveSteps* steps,
                     const char* where) {
    const int law = static_cast<int>(LeafLaw::TreeLeaf);
    int rc = integrator == TreeIntegrator::KickDriftKickAdaptive ? adaptive_steps(tree.plan, tree.ctx, law, NBX_REFERENCE_G, nsteps, rebuild_every, steps, where)
             : integrator == TreeIntegrator::KickDriftKick       ? nbx_leaf_plan_step_octree_kdk(tree.plan, tree.ctx, law, NBX_REFERENCE_G, dt, nsteps, rebuild_every)
                                                                 : nbx_leaf_plan_step_octree(tree.plan, tree.ctx, law, NBX_REFERENCE_G, dt, nsteps, rebuild_every);
    if (!rc) rc = nbx_ctx_download_bodies(tree.ctx, bodies.data(), sizeof(Body<D>));
    if (rc != NBX_OK) raise_leaf(where, rc);
}
}  // namespace

template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order, TreeIntegrator integrator,
                          TreeAdaptiveSteps* steps) {
    if (bodies.empty()) return;
    OctreeOnDevice<D> tree(bodies, theta, depth, "barnes_hut_hip_steps", -1, far_order);
    tree_leaf_steps<D>(tree, bodies, dt, nsteps, rebuild_every, integrator, steps, "barnes_hut_hip_steps");
}

namespace {
void check_capacity(int leaf_capacity, const char* where) {
    if (leaf_capacity < 0) throw std::runtime_error(std::string(where) + ": leaf_capacity must be >= 0");
}
}  // namespace

template <int D>
std::vector<Vector<D>> barnes_hut_hip_adaptive_n_body(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, int far_order) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_n_body");
    std::vector<Vector<D>> forces(bodies.size());
    if (bodies.empty()) return forces;
    OctreeOnDevice<D> tree(bodies, theta, max_depth, "barnes_hut_hip_adaptive_n_body", leaf_capacity, far_order);
    const int rc = nbx_leaf_plan_forces_ctx(tree.plan, tree.ctx, static_cast<int>(LeafLaw::TreeLeaf), NBX_REFERENCE_G, reinterpret_cast<double*>(forces.data()), nullptr);
    if (rc != NBX_OK) raise_leaf("barnes_hut_hip_adaptive_n_body", rc);
    return forces;
}

template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every, int far_order) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_steps");
    if (bodies.empty()) return;
    OctreeOnDevice<D> tree(bodies, theta, max_depth, "barnes_hut_hip_adaptive_steps", leaf_capacity, far_order);
    int rc = nbx_leaf_plan_step_octree(tree.plan, tree.ctx, static_cast<int>(LeafLaw::TreeLeaf), NBX_REFERENCE_G, dt, nsteps, rebuild_every);
    if (!rc) rc = nbx_ctx_download_bodies(tree.ctx, bodies.data(), sizeof(Body<D>));
    if (rc != NBX_OK) raise_leaf("barnes_hut_hip_adaptive_steps", rc);
}

template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every, int far_order,
                                   TreeIntegrator integrator, TreeAdaptiveSteps* steps) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_steps");
    if (bodies.empty()) return;
    OctreeOnDevice<D> tree(bodies, theta, max_depth, "barnes_hut_hip_adaptive_steps", leaf_capacity, far_order);
    tree_leaf_steps<D>(tree, bodies, dt, nsteps, rebuild_every, integrator, steps, "barnes_hut_hip_adaptive_steps");
}

template <int D>
void barnes_hut_hip_adaptive_leaves(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, std::size_t* n_leaves, std::size_t* largest_leaf) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_leaves");
    *n_leaves = *largest_leaf = 0;
    if (bodies.empty()) return;
    OctreeOnDevice<D> tree(bodies, theta, max_depth, "barnes_hut_hip_adaptive_leaves", leaf_capacity);
    int rc = nbx_leaf_plan_structure_sizes(tree.plan, n_leaves, nullptr, nullptr, nullptr);
    std::vector<std::uint32_t> offsets(*n_leaves + 1);
    if (!rc) rc = nbx_leaf_plan_get_structure(tree.plan, offsets.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != NBX_OK) raise_leaf("barnes_hut_hip_adaptive_leaves", rc);
    for (std::size_t l = 0; l < *n_leaves; ++l) *largest_leaf = std::max<std::size_t>(*largest_leaf, offsets[l + 1] - offsets[l]);
}

template <int D>
void barnes_hut_hip_tree_energy(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int depth, int far_order, double* kinetic, double* potential) {
    if (kinetic) *kinetic = 0.0;
    if (potential) *potential = 0.0;
    if (bodies.empty()) return;
    OctreeOnDevice<D> tree(bodies, theta, depth, "barnes_hut_hip_tree_energy", leaf_capacity, far_order);
    const int rc = nbx_leaf_plan_energy(tree.plan, tree.ctx, static_cast<int>(LeafLaw::TreeLeaf), NBX_REFERENCE_G, kinetic, potential);
    if (rc != NBX_OK) raise_leaf("barnes_hut_hip_tree_energy", rc);
}
template void barnes_hut_hip_tree_energy<2>(const std::vector<Body<2>>&, double, int, int, int, double*, double*);
template void barnes_hut_hip_tree_energy<3>(const std::vector<Body<3>>&, double, int, int, int, double*, double*);

// ---- softened Newtonian gravity through the tree ----
template <int D>
BarnesHutNewtonHip<D>::BarnesHutNewtonHip(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int depth, int far_order, double G, double epsilon)
    : n_(bodies.size()), G_(G) {
    const char* const where = "BarnesHutNewtonHip";
    if (bodies.empty()) throw std::runtime_error(std::string(where) + ": no bodies");
    int rc = nbx_ctx_create(&ctx_, leaf_device(), D, bodies.size(), 1, 0);
    if (!rc) rc = nbx_ctx_upload_bodies(ctx_, bodies.data(), sizeof(Body<D>));
    if (!rc && leaf_capacity >= 0) rc = nbx_leaf_plan_create_octree_adaptive(&plan_, ctx_, depth, leaf_capacity, theta);
    else if (!rc) rc = nbx_leaf_plan_create_octree(&plan_, ctx_, depth > 0 ? depth : barnes_hut_hip_depth(bodies.size(), D), theta);
    if (!rc) rc = nbx_leaf_plan_set_far_order(plan_, far_order);
    if (!rc) rc = nbx_leaf_plan_set_softening(plan_, epsilon);
    // the context's own law, for nbx_ctx_energy only: every force of this object is the plan's
    if (!rc) rc = nbx_ctx_set_softening(ctx_, epsilon);
    if (!rc) rc = nbx_ctx_set_law(ctx_, NBX_FORCE_LAW_NEWTON);
    if (rc != NBX_OK) {
        nbx_leaf_plan_destroy(plan_);
        nbx_ctx_destroy(ctx_);
        raise_leaf(where, rc);
    }
}
template <int D>
BarnesHutNewtonHip<D>::~BarnesHutNewtonHip() {
    nbx_leaf_plan_destroy(plan_);   // before the context, as in LeafPairSimulationHip
    nbx_ctx_destroy(ctx_);
}
template <int D>
std::vector<Vector<D>> BarnesHutNewtonHip<D>::forces() {
    std::vector<Vector<D>> out(n_);
    const int rc = nbx_leaf_plan_forces_ctx(plan_, ctx_, NBX_LAW_NEWTON, G_, reinterpret_cast<double*>(out.data()), nullptr);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::forces", rc);
    return out;
}
template <int D>
void BarnesHutNewtonHip<D>::step(double dt, int nsteps, int rebuild_every) {
    const int rc = nbx_leaf_plan_step_octree(plan_, ctx_, NBX_LAW_NEWTON, G_, dt, nsteps, rebuild_every);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::step", rc);
}
template <int D>
void BarnesHutNewtonHip<D>::step_kdk(double dt, int nsteps, int rebuild_every) {
    const int rc = nbx_leaf_plan_step_octree_kdk(plan_, ctx_, NBX_LAW_NEWTON, G_, dt, nsteps, rebuild_every);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::step_kdk", rc);
}
template <int D>
nbx_step_clock BarnesHutNewtonHip<D>::step_kdk_adaptive(const nbx_step_control& control, int max_steps, int rebuild_every) {
    nbx_step_clock clock{};
    clock.t = control.t_start;
    int rc = nbx_leaf_plan_step_kdk_adaptive(plan_, ctx_, NBX_LAW_NEWTON, G_, &control, max_steps, rebuild_every);
    if (!rc && max_steps > 0) rc = nbx_leaf_plan_get_step_clock(plan_, &clock);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::step_kdk_adaptive", rc);
    return clock;
}
template <int D>
void BarnesHutNewtonHip<D>::step_range(double* dt_smallest, double* dt_largest) {
    const int rc = adaptive_step_range(plan_, dt_smallest, dt_largest);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::step_range", rc);
}
template <int D>
double BarnesHutNewtonHip<D>::max_accel() {
    double a = 0.0;
    const int rc = nbx_leaf_plan_max_accel(plan_, &a);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::max_accel", rc);
    return a;
}
template <int D>
void BarnesHutNewtonHip<D>::energy(double* kinetic, double* potential) {
    const int rc = nbx_ctx_energy(ctx_, G_, kinetic, potential);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::energy", rc);
}
template <int D>
void BarnesHutNewtonHip<D>::tree_energy(double* kinetic, double* potential) {
    const int rc = nbx_leaf_plan_energy(plan_, ctx_, NBX_LAW_NEWTON, G_, kinetic, potential);
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::tree_energy", rc);
}
template <int D>
void BarnesHutNewtonHip<D>::download(std::vector<Body<D>>& bodies) {
    if (bodies.size() != n_) throw std::runtime_error("BarnesHutNewtonHip::download: body count differs");
    const int rc = nbx_ctx_download_bodies(ctx_, bodies.data(), sizeof(Body<D>));
    if (rc != NBX_OK) raise_leaf("BarnesHutNewtonHip::download", rc);
}
template class BarnesHutNewtonHip<2>;
template class BarnesHutNewtonHip<3>;

template <int D>
std::vector<Vector<D>> newton_all_pairs_forces_hip(const std::vector<Body<D>>& bodies, double G, double epsilon) {
    std::vector<Vector<D>> out(bodies.size());
    if (bodies.empty()) return out;
    nbx_ctx* ctx = nullptr;
    int rc = nbx_ctx_create(&ctx, leaf_device(), D, bodies.size(), 1, 0);
    if (!rc) rc = nbx_ctx_upload_bodies(ctx, bodies.data(), sizeof(Body<D>));
    if (!rc) rc = nbx_ctx_set_softening(ctx, epsilon);
    if (!rc) rc = nbx_ctx_set_law(ctx, NBX_FORCE_LAW_NEWTON);
    if (!rc) rc = nbx_ctx_compute_accel(ctx, NBX_SRC_ALL);
    if (!rc) rc = nbx_ctx_get_forces(ctx, G, reinterpret_cast<double*>(out.data()));
    nbx_ctx_destroy(ctx);
    if (rc != NBX_OK) raise_leaf("newton_all_pairs_forces_hip", rc);
    return out;
}
template std::vector<Vector<2>> newton_all_pairs_forces_hip<2>(const std::vector<Body<2>>&, double, double);
template std::vector<Vector<3>> newton_all_pairs_forces_hip<3>(const std::vector<Body<3>>&, double, double);

template <int D>
std::vector<Vector<D>> barnes_hut_hip_n_body(const std::vector<Body<D>>& bodies, double theta, int depth, int far_order, double G, double epsilon) {
    if (bodies.empty()) return {};
    return BarnesHutNewtonHip<D>(bodies, theta, -1, depth, far_order, G, epsilon).forces();
}
template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order, double G, double epsilon) {
    if (bodies.empty()) return;
    BarnesHutNewtonHip<D> sim(bodies, theta, -1, depth, far_order, G, epsilon);
    sim.step(dt, nsteps, rebuild_every);
    sim.download(bodies);
}
template <int D>
std::vector<Vector<D>> barnes_hut_hip_adaptive_n_body(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, int far_order, double G,
                                                      double epsilon) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_n_body");
    if (bodies.empty()) return {};
    return BarnesHutNewtonHip<D>(bodies, theta, leaf_capacity, max_depth, far_order, G, epsilon).forces();
}
template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every,
                                   int far_order, double G, double epsilon) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_steps");
    if (bodies.empty()) return;
    BarnesHutNewtonHip<D> sim(bodies, theta, leaf_capacity, max_depth, far_order, G, epsilon);
    sim.step(dt, nsteps, rebuild_every);
    sim.download(bodies);
}
namespace {
// the Newtonian object's step loop under any integrator
template <int D>
void newton_steps(BarnesHutNewtonHip<D>& sim, double dt, int nsteps, int rebuild_every, TreeIntegrator integrator, TreeAdaptiveSteps* steps, const char* where) {
    if (integrator == TreeIntegrator::KickDriftKickAdaptive) {
        if (!steps) throw std::runtime_error(std::string(where) + ": TreeIntegrator::KickDriftKickAdaptive needs its TreeAdaptiveSteps");
        steps->clock = sim.step_kdk_adaptive(steps->control, nsteps, rebuild_every);
        steps->dt_smallest = steps->dt_largest = 0.0;
        if (nsteps > 0) sim.step_range(&steps->dt_smallest, &steps->dt_largest);
    } else if (integrator == TreeIntegrator::KickDriftKick) {
        sim.step_kdk(dt, nsteps, rebuild_every);
    } else {
        sim.step(dt, nsteps, rebuild_every);
    }
}
}  // namespace

template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order, double G, double epsilon,
                          TreeIntegrator integrator, TreeAdaptiveSteps* steps) {
    if (bodies.empty()) return;
    BarnesHutNewtonHip<D> sim(bodies, theta, -1, depth, far_order, G, epsilon);
    newton_steps<D>(sim, dt, nsteps, rebuild_every, integrator, steps, "barnes_hut_hip_steps");
    sim.download(bodies);
}
template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every,
                                   int far_order, double G, double epsilon, TreeIntegrator integrator, TreeAdaptiveSteps* steps) {
    check_capacity(leaf_capacity, "barnes_hut_hip_adaptive_steps");
    if (bodies.empty()) return;
    BarnesHutNewtonHip<D> sim(bodies, theta, leaf_capacity, max_depth, far_order, G, epsilon);
    newton_steps<D>(sim, dt, nsteps, rebuild_every, integrator, steps, "barnes_hut_hip_adaptive_steps");
    sim.download(bodies);
}
template void barnes_hut_hip_steps<2>(std::vector<Body<2>>&, double, int, double, int, int, int, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_steps<3>(std::vector<Body<3>>&, double, int, double, int, int, int, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_adaptive_steps<2>(std::vector<Body<2>>&, double, int, int, double, int, int, int, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_adaptive_steps<3>(std::vector<Body<3>>&, double, int, int, double, int, int, int, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_steps<2>(std::vector<Body<2>>&, double, int, double, int, int, int, double, double, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_steps<3>(std::vector<Body<3>>&, double, int, double, int, int, int, double, double, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_adaptive_steps<2>(std::vector<Body<2>>&, double, int, int, double, int, int, int, double, double, TreeIntegrator, TreeAdaptiveSteps*);
template void barnes_hut_hip_adaptive_steps<3>(std::vector<Body<3>>&, double, int, int, double, int, int, int, double, double, TreeIntegrator, TreeAdaptiveSteps*);
template std::vector<Vector<2>> barnes_hut_hip_n_body<2>(const std::vector<Body<2>>&, double, int, int, double, double);
template std::vector<Vector<3>> barnes_hut_hip_n_body<3>(const std::vector<Body<3>>&, double, int, int, double, double);
template void barnes_hut_hip_steps<2>(std::vector<Body<2>>&, double, int, double, int, int, int, double, double);
template void barnes_hut_hip_steps<3>(std::vector<Body<3>>&, double, int, double, int, int, int, double, double);
template std::vector<Vector<2>> barnes_hut_hip_adaptive_n_body<2>(const std::vector<Body<2>>&, double, int, int, int, double, double);
template std::vector<Vector<3>> barnes_hut_hip_adaptive_n_body<3>(const std::vector<Body<3>>&, double, int, int, int, double, double);
template void barnes_hut_hip_adaptive_steps<2>(std::vector<Body<2>>&, double, int, int, double, int, int, int, double, double);
template void barnes_hut_hip_adaptive_steps<3>(std::vector<Body<3>>&, double, int, int, double, int, int, int, double, double);

template std::vector<Vector<2>> barnes_hut_hip_adaptive_n_body<2>(const std::vector<Body<2>>&, double, int, int, int);
template std::vector<Vector<3>> barnes_hut_hip_adaptive_n_body<3>(const std::vector<Body<3>>&, double, int, int, int);
template void barnes_hut_hip_adaptive_steps<2>(std::vector<Body<2>>&, double, int, int, double, int, int, int);
template void barnes_hut_hip_adaptive_steps<3>(std::vector<Body<3>>&, double, int, int, double, int, int, int);
template void barnes_hut_hip_adaptive_leaves<2>(const std::vector<Body<2>>&, double, int, int, std::size_t*, std::size_t*);
template void barnes_hut_hip_adaptive_leaves<3>(const std::vector<Body<3>>&, double, int, int, std::size_t*, std::size_t*);
template std::vector<Vector<2>> barnes_hut_hip_n_body<2>(const std::vector<Body<2>>&, double, int, int);
template std::vector<Vector<3>> barnes_hut_hip_n_body<3>(const std::vector<Body<3>>&, double, int, int);
template void barnes_hut_hip_steps<2>(std::vector<Body<2>>&, double, int, double, int, int, int);
template void barnes_hut_hip_steps<3>(std::vector<Body<3>>&, double, int, double, int, int, int);

template <int D>
LeafLists build_uniform_leaves(const std::vector<Body<D>>& bodies, int depth) {
    LeafLists L;
    const std::size_t n = bodies.size();
    if (n == 0) return L;
    const long long g = 1LL << depth;
    Vector<D> lo = bodies[0].position, hi = bodies[0].position;
    for (const auto& b : bodies)
        for (int d = 0; d < D; ++d) { lo[d] = std::min(lo[d], b.position[d]); hi[d] = std::max(hi[d], b.position[d]); }
    double half = 0.0;
    Vector<D> centre;
    for (int d = 0; d < D; ++d) { centre[d] = (lo[d] + hi[d]) / 2.0; half = std::max(half, (hi[d] - lo[d]) / 2.0); }
    half = std::max(half * 1.01, 1e-300);
    auto cell_of = [&](const Body<D>& b, long long* c) {
        for (int d = 0; d < D; ++d) {
            long long k = (long long)std::floor((b.position[d] - (centre[d] - half)) / (2.0 * half) * (double)g);
            c[d] = std::min(std::max(k, 0LL), g - 1);
        }
    };
    auto key_of = [&](const long long* c) { long long k = 0; for (int d = 0; d < D; ++d) k = k * g + c[d]; return k; };
    std::vector<long long> key(n);
    for (std::size_t i = 0; i < n; ++i) { long long c[3]; cell_of(bodies[i], c); key[i] = key_of(c); }
    std::vector<std::uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](std::uint32_t a, std::uint32_t b) { return key[a] < key[b]; });
    L.leaf_bodies = order;
    L.leaf_offsets.clear();
    std::vector<long long> leaf_key;
    std::unordered_map<long long, std::uint32_t> index_of;
    for (std::size_t s = 0; s < n; ++s)
        if (s == 0 || key[order[s]] != key[order[s - 1]]) {
            index_of[key[order[s]]] = (std::uint32_t)leaf_key.size();
            leaf_key.push_back(key[order[s]]);
            L.leaf_offsets.push_back((std::uint32_t)s);
        }
    L.leaf_offsets.push_back((std::uint32_t)n);
    L.list_offsets.assign(1, 0u);
    int n_off = 1;
    for (int d = 0; d < D; ++d) n_off *= 3;
    for (std::size_t l = 0; l < leaf_key.size(); ++l) {
        long long c[3] = {0, 0, 0}, rest = leaf_key[l];
        for (int d = D - 1; d >= 0; --d) { c[d] = rest % g; rest /= g; }
        L.list_sources.push_back((std::uint32_t)l);  // own bodies first
        for (int o = 0; o < n_off; ++o) {            // offsets in the same order as leaves.py (first axis slowest)
            long long q[3], t = o;
            bool self = true, inside = true;
            for (int d = D - 1; d >= 0; --d) { const long long off = t % 3 - 1; t /= 3; q[d] = c[d] + off; self = self && off == 0; inside = inside && q[d] >= 0 && q[d] < g; }
            if (self || !inside) continue;
            const auto it = index_of.find(key_of(q));
            if (it != index_of.end()) L.list_sources.push_back(it->second);
        }
        L.list_offsets.push_back((std::uint32_t)L.list_sources.size());
    }
    return L;
}

template <int D>
LeafLists build_octree_cells(const std::vector<Body<D>>& bodies, int depth, double theta) {
    LeafLists L;
    L.far_offsets.assign(1, 0u);
    const std::size_t n = bodies.size();
    if (n == 0) return L;
    const long long g = 1LL << depth;
    Vector<D> lo = bodies[0].position, hi = bodies[0].position;
    for (const auto& b : bodies)
        for (int d = 0; d < D; ++d) { lo[d] = std::min(lo[d], b.position[d]); hi[d] = std::max(hi[d], b.position[d]); }
    double half = 0.0;
    Vector<D> centre;
    for (int d = 0; d < D; ++d) { centre[d] = (lo[d] + hi[d]) / 2.0; half = std::max(half, (hi[d] - lo[d]) / 2.0); }
    half = std::max(half * 1.01, 1e-300);
    // Morton key: bit b of axis d at bit b * D + (D - 1 - d)
    std::vector<long long> key(n);
    for (std::size_t i = 0; i < n; ++i) {
        long long k = 0;
        for (int d = 0; d < D; ++d) {
            long long c = (long long)std::floor((bodies[i].position[d] - (centre[d] - half)) / (2.0 * half) * (double)g);
            c = std::min(std::max(c, 0LL), g - 1);
            for (int bit = 0; bit < depth; ++bit) k |= ((c >> bit) & 1LL) << (bit * D + (D - 1 - d));
        }
        key[i] = k;
    }
    std::vector<std::uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](std::uint32_t a, std::uint32_t b) { return key[a] < key[b]; });
    L.leaf_bodies = order;
    L.leaf_offsets.clear();
    std::vector<long long> leaf_key;
    for (std::size_t s = 0; s < n; ++s)
        if (s == 0 || key[order[s]] != key[order[s - 1]]) { leaf_key.push_back(key[order[s]]); L.leaf_offsets.push_back((std::uint32_t)s); }
    L.leaf_offsets.push_back((std::uint32_t)n);
    const std::size_t nl = leaf_key.size();
    // the non-empty nodes of levels 1 .. depth: keys (sorted), leaf ranges, the id of the level's first cell
    std::vector<std::vector<long long>> lv_key(depth + 1);
    std::vector<std::size_t> lv_base(depth + 2, 0);
    for (int lv = 1; lv <= depth; ++lv) {
        lv_base[lv] = L.cell_first_leaf.size();
        for (std::size_t l = 0; l < nl; ++l) {
            const long long k = leaf_key[l] >> (D * (depth - lv));
            if (lv_key[lv].empty() || lv_key[lv].back() != k) { lv_key[lv].push_back(k); L.cell_first_leaf.push_back((std::uint32_t)l); L.cell_leaf_count.push_back(0u); }
            ++L.cell_leaf_count.back();
        }
    }
    auto coords = [&](long long k, int lv, long long* c) {
        for (int d = 0; d < D; ++d) {
            c[d] = 0;
            for (int bit = 0; bit < lv; ++bit) c[d] |= ((k >> (bit * D + (D - 1 - d))) & 1LL) << bit;
        }
    };
    L.list_offsets.assign(1, 0u);
    std::vector<std::size_t> frontier, next;
    for (std::size_t t = 0; t < nl; ++t) {
        if (depth == 0) { L.list_sources.push_back((std::uint32_t)t); L.list_offsets.push_back((std::uint32_t)L.list_sources.size()); L.far_offsets.push_back(0u); continue; }
        long long q[3];
        coords(leaf_key[t], depth, q);
        frontier.resize(lv_key[1].size());
        std::iota(frontier.begin(), frontier.end(), (std::size_t)0);
        L.list_sources.push_back((std::uint32_t)t);                       // the leaf itself first
        for (int lv = 1; lv <= depth; ++lv) {
            const int s = depth - lv;
            next.clear();
            for (const std::size_t node : frontier) {
                long long c[3], gap2 = 0;
                coords(lv_key[lv][node], lv, c);
                for (int d = 0; d < D; ++d) {
                    const long long blo = c[d] << s;
                    const long long gd = std::max(0LL, std::max(blo - (q[d] + 1), q[d] - (blo + (1LL << s))));
                    gap2 += gd * gd;
                }
                if ((double)(1LL << s) < theta * std::sqrt((double)gap2)) { L.far_cells.push_back((std::uint32_t)(lv_base[lv] + node)); continue; }
                if (lv == depth) { if (node != t) L.list_sources.push_back((std::uint32_t)node); continue; }
                const auto& kids = lv_key[lv + 1];
                const std::size_t k0 = (std::size_t)(std::lower_bound(kids.begin(), kids.end(), lv_key[lv][node] << D) - kids.begin());
                const std::size_t k1 = (std::size_t)(std::lower_bound(kids.begin(), kids.end(), (lv_key[lv][node] + 1) << D) - kids.begin());
                for (std::size_t k = k0; k < k1; ++k) next.push_back(k);
            }
            frontier.swap(next);
        }
        L.list_offsets.push_back((std::uint32_t)L.list_sources.size());
        L.far_offsets.push_back((std::uint32_t)L.far_cells.size());
    }
    return L;
}

// The cell index, the keys and the acceptance test must round as numpy's two-step arithmetic does: no fused multiply-adds from here on.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

template <int D>
LeafLists build_adaptive_octree_cells(const std::vector<Body<D>>& bodies, int max_depth, int leaf_capacity, double theta) {
    namespace ot = nbx_octree;
    if (max_depth < 0 || max_depth > ot::kMaxDepth || leaf_capacity < 0 || !(theta >= 0.0) || !std::isfinite(theta))
        throw std::invalid_argument("build_adaptive_octree_cells: max_depth in [0, 10], leaf_capacity >= 0, theta finite and >= 0");
    LeafLists L;
    L.far_offsets.assign(1, 0u);
    const std::size_t n = bodies.size(), cap = (std::size_t)leaf_capacity;
    if (n == 0) return L;
    const int depth = max_depth;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (int d = 0; d < D; ++d) lo[d] = hi[d] = bodies[0].position[d];
    for (const auto& b : bodies)
        for (int d = 0; d < D; ++d) { lo[d] = std::min(lo[d], b.position[d]); hi[d] = std::max(hi[d], b.position[d]); }
    const ot::RootBox box = ot::root_box(lo, hi, D);
    std::vector<std::uint32_t> key(n);
    for (std::size_t i = 0; i < n; ++i) {
        double x[3] = {0, 0, 0};
        for (int d = 0; d < D; ++d) x[d] = bodies[i].position[d];
        key[i] = ot::body_key(x, box, D, depth);
    }
    std::vector<std::uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](std::uint32_t a, std::uint32_t b) { return key[a] < key[b]; });
    L.leaf_bodies = order;
    if (!ot::root_is_split(n, depth, cap)) {                       // one leaf, its near list itself, no cells
        L.leaf_offsets = {0u, (std::uint32_t)n};
        L.list_offsets = {0u, 1u};
        L.list_sources = {0u};
        L.far_offsets = {0u, 0u};
        return L;
    }
    // the finest level's runs, and every run's leaf level: the first level whose node holds at most `cap` bodies, else max_depth
    std::vector<std::uint32_t> run_key, run_off;
    for (std::size_t s = 0; s < n; ++s)
        if (s == 0 || key[order[s]] != key[order[s - 1]]) { run_key.push_back(key[order[s]]); run_off.push_back((std::uint32_t)s); }
    run_off.push_back((std::uint32_t)n);
    const std::size_t nr = run_key.size();
    std::vector<int> run_level(nr, 0);
    for (int lv = 1; lv <= depth; ++lv) {
        const int shift = D * (depth - lv);
        for (std::size_t r = 0; r < nr;) {
            std::size_t e = r + 1;
            while (e < nr && (run_key[e] >> shift) == (run_key[r] >> shift)) ++e;
            const bool leaf = lv == depth || (cap > 0 && run_off[e] - run_off[r] <= cap);
            for (std::size_t i = r; i < e; ++i)
                if (run_level[i] == 0 && leaf) run_level[i] = lv;
            r = e;
        }
    }
    std::vector<std::uint32_t> leaf_key;
    std::vector<int> leaf_level;
    L.leaf_offsets.clear();
    for (std::size_t r = 0; r < nr; ++r) {
        const int shift = D * (depth - run_level[r]);
        if (r == 0 || (run_key[r] >> shift) != (run_key[r - 1] >> shift)) { leaf_key.push_back(run_key[r]); leaf_level.push_back(run_level[r]); L.leaf_offsets.push_back(run_off[r]); }
    }
    L.leaf_offsets.push_back((std::uint32_t)n);
    const std::size_t nl = leaf_key.size();
    // the existing nodes of levels 1 .. depth: prefix, first leaf, leaf count, leaf or split, the id of the level's first cell
    struct Level { std::vector<std::uint32_t> key, first, count; std::vector<char> leaf; std::size_t base = 0; };
    std::vector<Level> lv_of(depth + 2);
    for (int lv = 1; lv <= depth; ++lv) {
        Level& V = lv_of[lv];
        V.base = L.cell_first_leaf.size();
        const int shift = D * (depth - lv);
        for (std::size_t l = 0; l < nl; ++l) {
            if (leaf_level[l] < lv) continue;
            const std::uint32_t k = leaf_key[l] >> shift;
            if (V.key.empty() || V.key.back() != k) { V.key.push_back(k); V.first.push_back((std::uint32_t)l); V.count.push_back(0u); V.leaf.push_back(leaf_level[l] == lv); }
            ++V.count.back();
        }
        L.cell_first_leaf.insert(L.cell_first_leaf.end(), V.first.begin(), V.first.end());
        L.cell_leaf_count.insert(L.cell_leaf_count.end(), V.count.begin(), V.count.end());
    }
    L.list_offsets.assign(1, 0u);
    std::vector<std::size_t> frontier, next;
    std::vector<std::uint32_t> others;
    for (std::size_t t = 0; t < nl; ++t) {
        const int st = depth - leaf_level[t];
        const std::uint32_t q = ot::packed_coords(leaf_key[t] >> (D * st), D, leaf_level[t]);
        frontier.resize(lv_of[1].key.size());
        std::iota(frontier.begin(), frontier.end(), (std::size_t)0);
        others.clear();
        for (int lv = 1; lv <= depth && !frontier.empty(); ++lv) {
            const Level& V = lv_of[lv];
            next.clear();
            for (const std::size_t node : frontier) {
                if (ot::accepts_box(q, st, ot::packed_coords(V.key[node], D, lv), D, depth - lv, theta)) { L.far_cells.push_back((std::uint32_t)(V.base + node)); continue; }
                if (V.leaf[node]) { if (V.first[node] != t) others.push_back(V.first[node]); continue; }
                const auto& kids = lv_of[lv + 1].key;
                const std::size_t k0 = (std::size_t)(std::lower_bound(kids.begin(), kids.end(), V.key[node] << D) - kids.begin());
                const std::size_t k1 = (std::size_t)(std::lower_bound(kids.begin(), kids.end(), (V.key[node] + 1u) << D) - kids.begin());
                for (std::size_t k = k0; k < k1; ++k) next.push_back(k);
            }
            frontier.swap(next);
        }
        std::sort(others.begin(), others.end());
        L.list_sources.push_back((std::uint32_t)t);                       // the leaf itself first, the others in leaf order
        L.list_sources.insert(L.list_sources.end(), others.begin(), others.end());
        L.list_offsets.push_back((std::uint32_t)L.list_sources.size());
        L.far_offsets.push_back((std::uint32_t)L.far_cells.size());
    }
    return L;
}

template LeafLists build_adaptive_octree_cells<2>(const std::vector<Body<2>>&, int, int, double);
template LeafLists build_adaptive_octree_cells<3>(const std::vector<Body<3>>&, int, int, double);
template LeafLists build_octree_cells<2>(const std::vector<Body<2>>&, int, double);
template LeafLists build_octree_cells<3>(const std::vector<Body<3>>&, int, double);
template std::vector<Vector<2>> leaf_pair_direct_forces_hip<2>(const std::vector<Body<2>>&, const LeafLists&, LeafLaw);
template std::vector<Vector<3>> leaf_pair_direct_forces_hip<3>(const std::vector<Body<3>>&, const LeafLists&, LeafLaw);
template LeafLists build_uniform_leaves<2>(const std::vector<Body<2>>&, int);
template LeafLists build_uniform_leaves<3>(const std::vector<Body<3>>&, int);
