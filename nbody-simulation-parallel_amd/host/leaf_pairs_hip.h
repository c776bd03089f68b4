// leaf_pairs_hip.h -- host-side mirror of the tree codes' direct (near-field) sums, backed by nbx_leaf_pair_forces
// (include/nbody_hip.h).  In the reference this step is FMM_Parlay<D>::p2p_phase(forces, bodies)
// (nbody-sim-new/fmm_parlay.cpp:916-1022, tree held by the object), the BVH leaf loop (bvh.cpp:150-176) and the
// octree leaf term (octree.cpp:105-125); here the tree is handed over as CSR leaf lists so that any tree can feed it.
#ifndef NBODY_AMD_LEAF_PAIRS_HIP_H
#define NBODY_AMD_LEAF_PAIRS_HIP_H

#include <cstdint>
#include <vector>

#include "nbody_hip.h"   // nbx_step_control, nbx_step_clock: what the adaptive step loops take and return

#if __has_include("nbody_types.h")
#include "nbody_types.h"
#else
#include "body.h"
#include "vector.h"
#endif

// leaf l owns bodies leaf_bodies[leaf_offsets[l] .. leaf_offsets[l+1]); target leaf t sums over the source leaves
// list_sources[list_offsets[t] .. list_offsets[t+1]) (own leaf included explicitly, fmm_parlay.cpp:973-974).
// The far field (optional; nbx_leaf_plan_set_cells): cell c is the leaves [cell_first_leaf[c], cell_first_leaf[c] + cell_leaf_count[c]);
// target leaf t is attracted by the cells far_cells[far_offsets[t] .. far_offsets[t+1]) as by one pseudo-body each (total mass at
// the centre of mass: octree.cpp:129-151, bvh.cpp:203-239).  Empty cell arrays: no far field.
struct LeafLists {
    std::vector<std::uint32_t> leaf_offsets{0}, leaf_bodies, list_offsets{0}, list_sources;
    std::vector<std::uint32_t> cell_first_leaf, cell_leaf_count, far_offsets, far_cells;
    std::size_t leaves() const { return leaf_offsets.size() - 1; }
    std::size_t cells() const { return cell_first_leaf.size(); }
};

enum class LeafLaw : int {
    Brute = 0,     // methods.cpp:21-37   repulsive, r^2 < 1e-10 skipped
    TreeLeaf = 1,  // octree.cpp:105-125, bvh.cpp:150-176   attractive, r^2 < 1e-9 skipped
    FmmP2P = 2,    // fmm_parlay.cpp:992-1020   attractive, identical positions skipped, r^2 < 1e-10 smoothed by (1e-5)^2
    Newton = 3     // extension (NBX_LAW_NEWTON): attractive m_j d / (r^2 + eps^2)^(3/2), every pair counted; plans only, needs set_softening
};

// Forces from the listed leaf pairs only (zero for bodies in no leaf).  Throws std::runtime_error on invalid lists or
// any device failure, like the solver wrappers of methods_hip.h; there is no CPU fallback.
template <int D>
std::vector<Vector<D>> leaf_pair_direct_forces_hip(const std::vector<Body<D>>& bodies, const LeafLists& lists, LeafLaw law);

// The same sums for a tree that STANDS while the bodies move -- the reference's call pattern: bvh.cpp:143-176 evaluates the
// leaf sums of a built BVH in every force evaluation, fmm_parlay.cpp:916-1022 once per step.  The structure is validated, laid
// out and uploaded once (nbx_leaf_plan_*; with the lists' cells and far lists, if any: every evaluation then carries near + far), the bodies live on the device (a context), and every evaluation only re-gathers
// positions and runs the pair kernel.  Every method throws std::runtime_error on failure; no CPU fallback.
template <int D>
class LeafPairSimulationHip {
public:
    LeafPairSimulationHip(const std::vector<Body<D>>& bodies, const LeafLists& lists);
    ~LeafPairSimulationHip();
    LeafPairSimulationHip(const LeafPairSimulationHip&) = delete;
    LeafPairSimulationHip& operator=(const LeafPairSimulationHip&) = delete;
    // leaf sums of the bodies as they stand on the device, brought to the host
    std::vector<Vector<D>> forces(LeafLaw law, double G);
    // the same evaluation with the sums left on the device; returns after the device has finished (wall-clock friendly)
    void evaluate(LeafLaw law, double G);
    // nsteps x { leaf sums; update_body_velocities; update_body_positions } (methods.cpp:425-450) on the device, asynchronous
    void step(LeafLaw law, double G, double dt, int nsteps);
    // nsteps kick-drift-kick steps (nbx_leaf_plan_step_kdk; extension, second order): nsteps + 1 evaluations, positions and velocities at
    // one time afterwards, asynchronous
    void step_kdk(LeafLaw law, double G, double dt, int nsteps);
    // kick-drift-kick with every step chosen on the device from the evaluation just made (nbx_leaf_plan_step_kdk_adaptive): up to
    // max_steps steps towards control.t_end; returns the device's clock (which synchronises)
    nbx_step_clock step_kdk_adaptive(LeafLaw law, double G, const nbx_step_control& control, int max_steps);
    void synchronize();   // waits for the steps queued so far
    void download(std::vector<Body<D>>& bodies);
    // 0 (NBX_FAR_MONOPOLE, every object's start) or 1 (NBX_FAR_QUADRUPOLE): the far cells' second-order term (nbx_leaf_plan_set_far_order)
    void set_far_order(int order);
    // the softening length of LeafLaw::Newton (nbx_leaf_plan_set_softening): 0 (every object's start) or in [1e-6, 1e15]
    void set_softening(double epsilon);
    float single_launch_ms(LeafLaw law, double G);      // pair kernel of one evaluation
    float back_to_back_ms(LeafLaw law, int reps);      // measurement: mean of the second half of `reps` launches in a row
private:
    struct nbx_ctx* ctx_ = nullptr;
    struct nbx_leaf_plan* plan_ = nullptr;
    std::size_t n_ = 0;
};

// Fixed-depth subdivision of the bodies' bounding box (2^depth cells per axis, box padded like fmm.cpp:386-387):
// non-empty cells are the leaves, each leaf's list is itself followed by its non-empty adjacent cells -- the simplest
// tree that produces the reference's neighbour-list structure (fmm.cpp:455-476).
template <int D>
LeafLists build_uniform_leaves(const std::vector<Body<D>>& bodies, int depth);

// A fixed-depth octree (quadtree for D = 2) with near AND far lists, the twin of nbody_amd.leaves.octree_cells: leaves = the non-empty
// cells of the 2^depth grid in MORTON order (every node is a contiguous range of leaves), cells = the non-empty nodes of levels
// 1 .. depth, and per target leaf a top-down walk that sends a node to the far list when side(node) < theta * gap (gap: box-to-box
// distance between the leaf's grid box and the node's) and a leaf-level node that is not accepted to the near list, the leaf first.
template <int D>
LeafLists build_octree_cells(const std::vector<Body<D>>& bodies, int depth, double theta);

// An ADAPTIVE octree with near and far lists, the twin of nbody_amd.leaves.adaptive_octree_cells and the specification of
// nbx_leaf_plan_create_octree_adaptive: root box, finest cells, Morton keys and body order of build_octree_cells(depth = max_depth);
// the root is split when max_depth >= 1 and (leaf_capacity == 0 or n > leaf_capacity); a node exists when it is not empty and its
// parent is split; an existing node is a leaf at max_depth or, for leaf_capacity > 0, with at most leaf_capacity bodies.  Leaves in
// Morton order, cells = the existing nodes of levels 1 .. max_depth level by level, and a walk per target leaf with the leaf's own
// box (octree_device.h accepts_box).  leaf_capacity = 0 gives build_octree_cells's arrays.  Throws std::invalid_argument for
// max_depth outside [0, 10], a negative capacity or a theta that is negative or not finite.
template <int D>
LeafLists build_adaptive_octree_cells(const std::vector<Body<D>>& bodies, int max_depth, int leaf_capacity, double theta);

// Barnes-Hut with the tree built ON THE DEVICE, in the shape of the reference's barnes_hut_seq_n_body (methods.h:47): bodies in,
// forces out, a new tree per call (methods.cpp:377-401).  The bodies go to a context, the fixed-depth octree, its near and far
// lists and the plan's layout are made there (nbx_leaf_plan_create_octree), one evaluation under the tree-leaf law with the
// reference's G follows, and the forces come back.  depth = 0 picks the smallest depth with at most 16 bodies per cell on
// average (barnes_hut_hip_depth), capped at 10.  far_order (here and in the three calls below): 0 = NBX_FAR_MONOPOLE, the reference's
// pseudo-bodies; 1 = NBX_FAR_QUADRUPOLE adds the cells' second-order term (nbx_leaf_plan_set_far_order).  Throws std::runtime_error on
// failure; no CPU fallback.
template <int D>
std::vector<Vector<D>> barnes_hut_hip_n_body(const std::vector<Body<D>>& bodies, double theta = 0.5, int depth = 0, int far_order = 0);
int barnes_hut_hip_depth(std::size_t n_bodies, int dim);
// nsteps x { rebuild the tree when step % rebuild_every == 0; forces; update_body_velocities; update_body_positions } on the device
// (nbx_leaf_plan_step_octree), the bodies brought back at the end.
template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every = 1, int far_order = 0);

// The same two calls over the ADAPTIVE octree (nbx_leaf_plan_create_octree_adaptive): leaves of at most leaf_capacity bodies down to
// max_depth.  The tree for inputs whose density varies -- a Plummer sphere's centre -- where a fixed depth leaves cells of thousands.
template <int D>
std::vector<Vector<D>> barnes_hut_hip_adaptive_n_body(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth = 10, int far_order = 0);
template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every = 1, int far_order = 0);
// leaves and largest leaf of the adaptive tree the device builds from `bodies` (what nbody_sim --leaf-cap reports)
template <int D>
void barnes_hut_hip_adaptive_leaves(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, std::size_t* n_leaves, std::size_t* largest_leaf);

// The integrator of the step loops below.  KickDrift is the reference helpers' order and what every signature without an integrator
// means; KickDriftKick is the synchronised second-order leapfrog (nbx_leaf_plan_step_octree_kdk: nsteps + 1 evaluations, the tree
// built again before evaluation e when e % rebuild_every == 0, positions and velocities at one time afterwards).
// KickDriftKickAdaptive is that loop with every step chosen on the device (nbx_leaf_plan_step_kdk_adaptive): it needs `steps`, whose
// control says how; dt is not read (control.dt_max bounds the steps) and nsteps is the cap on their number.
enum class TreeIntegrator { KickDrift, KickDriftKick, KickDriftKickAdaptive };
// What KickDriftKickAdaptive takes (control) and gives back: the device's clock and the smallest and largest step it took
// (both 0 when it took none).
struct TreeAdaptiveSteps {
    nbx_step_control control{};
    nbx_step_clock clock{};
    double dt_smallest = 0.0, dt_largest = 0.0;
};
template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order, TreeIntegrator integrator,
                          TreeAdaptiveSteps* steps = nullptr);
template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every, int far_order,
                                   TreeIntegrator integrator, TreeAdaptiveSteps* steps = nullptr);

// ---- softened Newtonian gravity through the tree (extension; NBX_LAW_NEWTON) ----
// The four calls above under F_i = +G m_i sum_j m_j d / (r^2 + epsilon^2)^(3/2): the same trees, lists and far orders, with the
// caller's G and a softening length epsilon > 0 (nbx_leaf_plan_set_softening).  Throw std::runtime_error on failure, epsilon = 0 included.
template <int D>
std::vector<Vector<D>> barnes_hut_hip_n_body(const std::vector<Body<D>>& bodies, double theta, int depth, int far_order, double G, double epsilon);
template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order, double G, double epsilon);
template <int D>
std::vector<Vector<D>> barnes_hut_hip_adaptive_n_body(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, int far_order, double G,
                                                      double epsilon);
template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every,
                                   int far_order, double G, double epsilon);
template <int D>
void barnes_hut_hip_steps(std::vector<Body<D>>& bodies, double theta, int depth, double dt, int nsteps, int rebuild_every, int far_order, double G, double epsilon,
                          TreeIntegrator integrator, TreeAdaptiveSteps* steps = nullptr);
template <int D>
void barnes_hut_hip_adaptive_steps(std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int max_depth, double dt, int nsteps, int rebuild_every,
                                   int far_order, double G, double epsilon, TreeIntegrator integrator, TreeAdaptiveSteps* steps = nullptr);

// The same system kept on the device between chunks of steps: a context with the bodies and a plan with the octree built from them
// (leaf_capacity < 0: fixed depth, depth 0 = barnes_hut_hip_depth; otherwise the adaptive tree down to `depth`).  energy() is the
// context's (nbx_ctx_energy) under the Newtonian law and the same epsilon -- the context's own law and softening are set for that
// call alone; the forces and the steps are the plan's.  tree_energy() is the plan's (nbx_leaf_plan_energy): the potential through the
// tree's own near lists and far cells at the object's far order and epsilon, O(N log N) like a step, on the tree as it stands (it does
// not rebuild) -- an observer: the steps that follow give the bits they would have given without it.
template <int D>
class BarnesHutNewtonHip {
public:
    BarnesHutNewtonHip(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int depth, int far_order, double G, double epsilon);
    ~BarnesHutNewtonHip();
    BarnesHutNewtonHip(const BarnesHutNewtonHip&) = delete;
    BarnesHutNewtonHip& operator=(const BarnesHutNewtonHip&) = delete;
    std::vector<Vector<D>> forces();                          // of the bodies as they stand, on the tree as it stands
    void step(double dt, int nsteps, int rebuild_every = 1);  // nbx_leaf_plan_step_octree
    void step_kdk(double dt, int nsteps, int rebuild_every = 1);   // nbx_leaf_plan_step_octree_kdk: kick-drift-kick, x and v at one time afterwards
    // nbx_leaf_plan_step_kdk_adaptive: up to max_steps steps towards control.t_end, each chosen on the device; returns the clock
    // (which synchronises).  A caller who chains calls passes the last clock's t as control.t_start.
    nbx_step_clock step_kdk_adaptive(const nbx_step_control& control, int max_steps, int rebuild_every = 1);
    void step_range(double* dt_smallest, double* dt_largest);  // over the steps of the last adaptive call (nbx_leaf_plan_get_step_history); 0, 0 if none
    double max_accel();                                       // largest |F_i| / m_i of the last evaluation (nbx_leaf_plan_max_accel); synchronises
    void energy(double* kinetic, double* potential);          // synchronises
    void tree_energy(double* kinetic, double* potential);     // synchronises
    void download(std::vector<Body<D>>& bodies);
private:
    struct nbx_ctx* ctx_ = nullptr;
    struct nbx_leaf_plan* plan_ = nullptr;
    std::size_t n_ = 0;
    double G_ = 0.0;
};

// The energy of `bodies` through a Barnes-Hut tree built on the device under the REFERENCE law the tree rows above evaluate
// (NBX_LAW_TREE_LEAF, the reference's G): K = sum m v^2 / 2 and U = -(G / 2) sum_i m_i phi_i with phi over the tree's near lists and far
// cells (nbx_leaf_plan_energy).  leaf_capacity < 0: the fixed-depth tree (depth 0 = barnes_hut_hip_depth); otherwise the adaptive one down
// to `depth`.  The reference-law trees have no object that lives between steps, so this is a call like theirs: bodies in, a new tree.
template <int D>
void barnes_hut_hip_tree_energy(const std::vector<Body<D>>& bodies, double theta, int leaf_capacity, int depth, int far_order, double* kinetic, double* potential);

// The yardstick of the Newtonian rows: the same law summed over ALL pairs by a context (nbx_ctx_set_law(NBX_FORCE_LAW_NEWTON),
// nbx_ctx_set_softening, nbx_ctx_compute_accel, nbx_ctx_get_forces) -- no tree, no plan.
template <int D>
std::vector<Vector<D>> newton_all_pairs_forces_hip(const std::vector<Body<D>>& bodies, double G, double epsilon);

// kernel time of the most recent leaf_pair_direct_forces_hip call on this thread (ms)
float last_leaf_pair_kernel_ms();

#endif
