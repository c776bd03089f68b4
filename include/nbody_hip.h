/*
 * nbody_hip.h -- C ABI of libnbody_hip.so: the MI355X (gfx950) all-pairs force + kick/drift path.
 *
 * This is the drop-in boundary for ONE hot path of mathaiml5/NBody-simulation-parallel: the O(N^2)
 * brute-force force evaluation and the two integrator helpers.  The reference has no FFI; its
 * "plugin API" is the free-function template shape of nbody-sim-new/methods.h:29-37 and :85-91,
 * called from run_benchmark<D> (nbody-sim-new/main.cpp:137-140).  Every entry point below names the
 * reference interface it replaces.  C++ wrappers with the reference's exact signatures live in
 * nbody-simulation-parallel_amd/host/methods_hip.h; INTEGRATION.md shows the harness-side binding.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, opaque context handle, int status (0 = NBX_OK).
 *    No C++ types, no exceptions, no torch types cross this boundary.
 *  - Host body arrays are the reference's Body<D> memory (nbody-sim-new/body.h:8-11):
 *    double position[D]; double velocity[D]; double mass;  i.e. stride 56 B (D=3) / 40 B (D=2).
 *    Host force arrays are the reference's Vector<D> memory (vector.h:9-12): double[D] per body.
 *  - The device computes in fp32 on SoA arrays; positions and masses are rounded to fp32 at this
 *    boundary.  Returned forces are F_i = -(G m_i) * sum_j m_j (p_j - p_i)/r^4 with pairs of
 *    r^2 < 1e-10 skipped -- the reference law exactly as written (methods.cpp:21-37), including its
 *    sign and its extra power of r; G*m_i is applied in fp64.
 *  - PRECISION DEFAULT: the reference's arithmetic is fp64 (vector.h:9-12); every entry point below runs the
 *    MIXED MODE by default -- fp32 pair terms for every target, then an fp64 re-evaluation of the targets whose
 *    fp32 sum cannot be trusted to 1e-5 relative (nbx_ctx_set_refine) -- so that every body's force is within
 *    1e-5 relative of brute_force_seq_n_body on the same (fp32-representable) inputs.  nbx_set_default_refine
 *    changes the tolerance for contexts made afterwards; 0 = plain fp32 (a few bodies per 100,000 then miss 1e-5).
 *  - There is NO CPU fallback: without a usable HIP device every compute call fails with
 *    NBX_ERR_NO_DEVICE / NBX_ERR_HIP.
 */
#ifndef NBODY_HIP_H
#define NBODY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define NBX_ABI_VERSION 5   /* 5: + the measurement entries nbx_variant_kernel_symbol, nbx_ctx_enable_clock_stamps, nbx_ctx_shader_clock, nbx_measure_valu_ceiling (additions only); 2: + nbx_leaf_pair_forces, nbx_*_set_softening, nbx_*_set_law, nbx_node_verify_exchange, nbx_ctx_close_set_mode, nbx_ctx_kick_drift2, nbx_*_step_kdk; 3: + nbx_*_set_refine, nbx_ctx_refine_stats, the strict fp64 kernel variant (additions only); 4: mixed mode ON by default (nbx_set_default_refine), nbx_brute_force_forces_ex, nbx_node_refine_stats, the leaf plan (nbx_leaf_plan_*); nbx_leaf_pair_forces no longer reads NBX_LEAF_TIMING_REPS */

/* status codes */
enum {
    NBX_OK = 0,
    NBX_ERR_INVALID = 1,    /* bad argument (null pointer, dim not 2/3, shard out of range ...) */
    NBX_ERR_NO_DEVICE = 2,  /* no HIP device visible */
    NBX_ERR_HIP = 3,        /* a HIP runtime call failed; nbx_last_error_detail() has the text */
    NBX_ERR_ALLOC = 4,      /* device or host allocation failed */
    NBX_ERR_STATE = 5       /* call made in the wrong order (e.g. step before upload) */
};

/* nbody-sim-new/utils.h:21 -- the reference's G, for callers that do not carry their own. */
#define NBX_REFERENCE_G 4.471e-21
/* nbody-sim-new/methods.cpp:24 -- pairs with r^2 below this are skipped. */
#define NBX_R2_SKIP 1e-10

typedef struct nbx_ctx nbx_ctx;

/* ---- library --------------------------------------------------------------------------------- */
int nbx_abi_version(void);
const char* nbx_strerror(int status);
/* Text of the last HIP failure seen by the calling thread ("" if none). */
const char* nbx_last_error_detail(void);
int nbx_device_count(int* count);
/* One-time start-up of `device` (HIP runtime, code-object load, first launches; ~0.15 s) so that a harness
 * that times whole calls, like the reference's safely_execute (utils.h:87-104), does not charge it to the
 * first solver call -- the way OpenMP's thread pool is already up when the reference times its CPU rows. */
int nbx_warmup(int device);
/* The library keeps a few idle HIP streams per device, the RCCL communicators of destroyed nodes, the device allocations of the last
 * two destroyed contexts per device (up to 1 GiB each: a context of N = 2^20 bodies holds ~0.3 GB, most of it the mixed mode's fp64 sums), and the device allocation of
 * the last nbx_leaf_pair_forces call per device (up to 2 GiB), for the next
 * context / node / call on the same devices (creating a stream costs ~1.4 ms and destroying one up to 3 ms on this runtime,
 * a communicator set for 8 GPUs far more -- against a force evaluation of 0.07 ms at N = 1,000).  This gives them
 * back; a harness calls it before it exits.  Safe to call at any time; live contexts and nodes are not touched. */
int nbx_release_cached(void);
/* Process-wide precision default taken by every context, node and one-shot call created AFTER this call (thread-safe):
 * rel_tolerance = 0: plain fp32; otherwise the mixed mode of nbx_ctx_set_refine with this tolerance and sigma factor
 * (0 = the library's calibrated factor).  The library starts with (1e-5, 0): the north star's tolerance for every body.
 * Same argument ranges as nbx_ctx_set_refine (NBX_ERR_INVALID otherwise). */
int nbx_set_default_refine(double rel_tolerance, double sigma_factor);
int nbx_get_default_refine(double* rel_tolerance, double* sigma_factor);
/* The calibrated sigma factor the mixed mode uses for `dim` with the default (three-level) force kernel when the caller passes 0
 * (24 in 3D, 32 in 2D; tests pin it).  The two-level variant "fastpk_t8_w3_u4", selected by name, keeps round 3's 48 / 64. */
double nbx_refine_sigma_default(int dim);

/* ---- one-shot entry points (host memory in, host memory out) --------------------------------- */

/* Replaces brute_force_seq_n_body<D> / brute_force_omp_n_body_{1,2}<D>
 * (nbody-sim-new/methods.h:29-37; methods.cpp:7-42, 45-95, 98-136).
 * bodies: n x Body<dim>, body_stride_bytes = sizeof(Body<dim>) (56 or 40; larger strides allowed).
 * forces_out: n x Vector<dim> (n*dim doubles).  Runs pack -> H2D -> kernel -> D2H on `device`.
 * kernel_ms (optional) receives the force kernel's own duration (hipEvent), for roofline figures;
 * the wall time of the whole call is what the reference's safely_execute (utils.h:87-104) times. */
int nbx_brute_force_forces(const void* bodies, size_t n, int dim, size_t body_stride_bytes,
                           double G, int device, double* forces_out, float* kernel_ms);
/* The same call with the precision spelled out and a report of what ran.  rel_tolerance < 0: the process default
 * (nbx_set_default_refine); 0: plain fp32; > 0: mixed mode with this tolerance.  info (optional) receives:
 *   kernel_ms        the force kernel's device time (hipEvent pair around it);  refine_ms  that of the mixed mode's select /
 *                    fp64 / fold kernels that followed it (0 in plain fp32)
 *   refine_tolerance the tolerance that was in force (0: plain fp32, or the mixed mode does not apply to the kernel that ran)
 *   refine_selected  targets the selection rule listed;  refine_refined  targets re-evaluated in fp64 (always equal: the
 *                    fp64 pass has room for every target of the shard -- a long list costs time, never accuracy)
 *   variant          kernel variant that ran (nbx_variant_name);  close_set_mode  NBX_CLOSE_* of the evaluation */
typedef struct nbx_eval_info {
    float kernel_ms, refine_ms;
    double refine_tolerance;
    unsigned refine_selected, refine_refined;
    int variant, close_set_mode;
} nbx_eval_info;
int nbx_brute_force_forces_ex(const void* bodies, size_t n, int dim, size_t body_stride_bytes, double G, int device,
                              double rel_tolerance, double* forces_out, nbx_eval_info* info);

/* Replaces the loop  { f = brute_force_*_n_body(bodies); update_body_velocities(bodies, f, dt);
 * update_body_positions(bodies, dt); }  repeated nsteps times (methods.h:85-91; methods.cpp:425-450;
 * the reference defines the two helpers but never calls them -- SURVEY F6).  bodies is updated in
 * place (positions and velocities; masses untouched).  State stays on the device between steps. */
int nbx_leapfrog(void* bodies, size_t n, int dim, size_t body_stride_bytes,
                 double G, double dt, int nsteps, int device, float* kernel_ms_total);

/* ---- leaf-pair direct sums (the near-field step of the reference's tree codes) ------------
 * Replaces the pointer-chasing direct sums of FMM_Parlay<D>::p2p_phase (nbody-sim-new/fmm_parlay.cpp:916-1022),
 * of the BVH leaf loop (bvh.cpp:150-176) and of the Barnes-Hut octree's leaf term (octree.cpp:105-125): for every
 * target leaf t and every source leaf s on t's list, every body of t sums the pair terms of every body of s.
 *   leaf_offsets[n_leaves+1], leaf_bodies[leaf_offsets[n_leaves]]: leaf l owns the bodies (indices into `bodies`)
 *       leaf_bodies[leaf_offsets[l] .. leaf_offsets[l+1]); a body belongs to at most one leaf; leaves may be empty.
 *   list_offsets[n_leaves+1], list_sources[list_offsets[n_leaves]]: the source leaves of target leaf t, summed in
 *       list order (include t itself for the leaf's own bodies, like the reference's "self interactions",
 *       fmm_parlay.cpp:973-974).
 *   law: per-pair rule, all of the form  G m_i m_j d / r^4  with d = p_j - p_i:
 *       NBX_LAW_BRUTE      methods.cpp:21-37: force -= ...; pairs with r^2 < 1e-10 skipped (the brute-force law)
 *       NBX_LAW_TREE_LEAF  octree.cpp:105-125 / bvh.cpp:150-176: force += ...; pairs with r^2 < 1e-9 skipped
 *       NBX_LAW_FMM_P2P    fmm_parlay.cpp:992-1020: force += ...; identical positions (|d_k| <= 1e-14) skipped; for
 *                          r^2 < 1e-10 the magnitude uses r^2 + (1e-5)^2 while the direction stays d/|d|
 * forces_out: n x Vector<dim>, zero for bodies in no leaf.  fp32 pair terms on leaf-ordered source pairs, fp64 sums;
 * every index array is validated before the pair kernels follow it (NBX_ERR_INVALID: on the host for small structures; larger
 * ones are laid out ON THE DEVICE, csrc/leaf_plan_device.h, where every index is checked before it is dereferenced and the
 * refusal comes back with the layout's 64-byte summary).  kernel_ms (optional) receives the pair kernel's duration (hipEvent).
 * This one-shot form validates, lays out and uploads the structure on every call (2.4-3.1 ms at N = 2^20, 84 MB of it PCIe);
 * a tree code that evaluates its leaf sums every step from resident bodies uses the PLAN below. */
/* NBX_LAW_NEWTON is the plan's fourth law (below, "softened Newtonian gravity on a plan"); this one-shot call has no plan to carry
 * a softening length and refuses it with NBX_ERR_INVALID. */
enum { NBX_LAW_BRUTE = 0, NBX_LAW_TREE_LEAF = 1, NBX_LAW_FMM_P2P = 2, NBX_LAW_NEWTON = 3 };
int nbx_leaf_pair_forces(const void* bodies, size_t n, int dim, size_t body_stride_bytes,
                         const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves,
                         const uint32_t* list_offsets, const uint32_t* list_sources,
                         int law, double G, int device, double* forces_out, float* kernel_ms);

/* ---- device-resident leaf plan ---------------------------------------------------------------------------------------
 * The reference's tree codes evaluate their leaf sums in EVERY force evaluation, from bodies that stay where they are
 * (bvh.cpp:143-176 BVH::calculate_force per body over the leaves its traversal accepts; fmm_parlay.cpp:916-1022 p2p_phase per
 * step) while the leaf structure changes only when the tree is rebuilt.  A plan is that structure made resident: the CSR
 * arrays are validated ONCE, the launch is laid out once (leaf-ordered slots, copy runs, workgroup tables: on the device,
 * csrc/leaf_plan_device.h, or -- small structures -- on the host, csrc/leaf_plan.h; the two make the same plan word for word)
 * and stays on `device` with the buffers the kernels need; each evaluation then only re-gathers positions and runs the pair
 * kernel.  A caller that rebuilds its tree per evaluation, as the reference does (methods.cpp:377-401), makes a new plan per
 * evaluation: 0.5-1.2 ms at N = 2^20.  NBODY_HIP_LEAF_PLANNER=host|device in the environment forces one planner.
 * Arguments as for nbx_leaf_pair_forces.  A plan is bound to its device, dim and body count; not thread-safe. */
typedef struct nbx_leaf_plan nbx_leaf_plan;
int nbx_leaf_plan_create(nbx_leaf_plan** out, int device, int dim, size_t n_bodies,
                         const uint32_t* leaf_offsets, const uint32_t* leaf_bodies, size_t n_leaves,
                         const uint32_t* list_offsets, const uint32_t* list_sources);
int nbx_leaf_plan_destroy(nbx_leaf_plan* plan);
/* Host bodies in, host forces out (n_bodies x Vector<dim>; zero for bodies in no leaf): one H2D copy of the Body<dim> array,
 * gather, pair kernel, one D2H copy.  kernel_ms (optional): the pair kernel's duration. */
int nbx_leaf_plan_forces(nbx_leaf_plan* plan, const void* bodies, size_t body_stride_bytes, int law, double G,
                         double* forces_out, float* kernel_ms);
/* Bodies RESIDENT on the device: positions and masses are gathered from `ctx` (a single-shard context of n_bodies bodies on
 * the plan's device, dim as the plan's; its fp32 source copy as it stands after the last upload / kick-drift), everything is
 * ordered on the context's stream.  forces_out may be NULL: the sums then stay on the device for nbx_leaf_plan_get_forces /
 * nbx_leaf_plan_kick_drift and the call does not wait for the device (kernel_ms must be NULL too).  With forces_out or
 * kernel_ms the call synchronises the stream. */
int nbx_leaf_plan_forces_ctx(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, double* forces_out, float* kernel_ms);
/* Forces of the last evaluation (n_bodies x Vector<dim>) -- F = +-(G m_i) x the leaf sums, the law's sign.  Synchronises.  The masses
 * are read where that evaluation found them: after nbx_leaf_plan_forces_ctx the context must still exist. */
int nbx_leaf_plan_get_forces(nbx_leaf_plan* plan, double* forces_out);
/* update_body_velocities + update_body_positions (methods.cpp:425-450) of `ctx`'s bodies from the LAST evaluation's leaf sums
 * (law and G as given there), fp64, the arithmetic of nbx_ctx_kick_drift; bodies in no leaf drift with their velocity.
 * Asynchronous on the context's stream.  This is the stepping loop of a tree code (its far field: nbx_leaf_plan_set_cells; without cells it is zero): what `nbody_sim
 * -m p --steps k` runs. */
int nbx_leaf_plan_kick_drift(nbx_leaf_plan* plan, nbx_ctx* ctx, double dt);
/* nsteps x { nbx_leaf_plan_forces_ctx(plan, ctx, law, G, NULL, NULL); nbx_leaf_plan_kick_drift(plan, ctx, dt) } with the structure
 * standing (the loop of methods.cpp:425-450 around the leaf sums; same kernels, same arithmetic, same results), in one call:
 * the steps are queued ahead of the device without the two calls' event bookkeeping.  Asynchronous; afterwards the plan holds the
 * LAST step's sums (of the positions before that step's drift), as after the two calls.  nsteps >= 0. */
int nbx_leaf_plan_step(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, double dt, int nsteps);
/* MEASUREMENT entry (tools/, bench.py): the pair kernel launched `reps` times back to back on the bodies of the last
 * evaluation (same sums every time); mean_ms = mean duration of the second half of the launches -- the kernel with the clocks
 * up, which a single launch from idle does not see.  1 <= reps <= 1000.  Synchronises. */
int nbx_leaf_plan_time_kernel(nbx_leaf_plan* plan, int law, int reps, float* mean_ms);
/* Counts of the layout: padded slots, copy runs, workgroups, wave64 per workgroup (any pointer may be NULL). */
int nbx_leaf_plan_info(const nbx_leaf_plan* plan, size_t* slots, size_t* runs, size_t* workgroups, int* waves_per_workgroup);

/* ---- the far field of a plan: cells and far lists -----------------------------------------------------------------------
 * The other half of the reference's tree codes: a body is attracted by a far node as by ONE pseudo-body of the node's total mass
 * at its centre of mass (octree.cpp:129-151, bvh.cpp:203-239).  A plan may carry CELLS and, per target leaf, a FAR LIST of cells;
 * every evaluation (nbx_leaf_plan_forces, _forces_ctx, _step) then, on the evaluation's stream: gathers the positions, computes
 * every cell's mass and centre of mass from the positions as they stand NOW, runs the pair kernel, and adds, for every body of
 * every target leaf t and every cell c on t's far list, the law's pair term with the pseudo-body (com_c, M_c) as the source into the
 * same slot-ordered sums -- so nbx_leaf_plan_get_forces / _kick_drift / _step carry near + far without further change.  A plan
 * without cells behaves bit for bit as before.
 *   cell_first_leaf[n_cells], cell_leaf_count[n_cells]: cell c = leaves [first, first + count) -- with leaves numbered depth-first
 *       (or in Morton order) every node of a tree is such a range.  Cells may nest, overlap, be empty or cover only empty leaves.
 *   far_offsets[n_leaves + 1], far_cells[far_offsets[n_leaves]]: CSR over target leaves like the source lists; entries are summed
 *       in a fixed order, a repeated entry counts twice; a leaf may have a far list and no near list or the other way round.
 *   moments: M_c = sum m_j, com_c = sum m_j p_j / M_c over the bodies of the cell's leaves, in fp64 from the fp32 slot values
 *       (per-leaf sums first, then each cell sums its leaves': fixed order, no atomics, an error that does not grow with N; the tests
 *       hold the centre of mass to 2^-30 of the cell's largest coordinate and the mass to 2^-30 M, 1/64 of an fp32 ulp).  A cell with M_c == 0 contributes exactly
 *       zero, never a NaN (bvh.cpp:225 guards the same case).
 *   law: the evaluation's law applied to the pseudo-body as if it were a body -- same sign, same rule below the law's threshold.
 *       (The reference's far branches skip only at dist < 1e-9 and recurse otherwise; a cell that close to a target is on no
 *       sensible far list.)  The pseudo-body is fp32 on the device, like every source.
 * NBX_ERR_INVALID, before anything is launched, when a cell's range runs past n_leaves, a far entry is >= n_cells, the offsets do
 * not start at 0 or decrease, or a pointer needed for a non-empty array is null; the plan then keeps its previous cells.
 * Replaces the plan's cells and far lists (n_cells = 0 removes them; the other pointers may then be NULL); the arrays are copied
 * (4 bytes per far entry go to the device); the call waits for the plan's last evaluation and for its own copies. */
int nbx_leaf_plan_set_cells(nbx_leaf_plan* plan, const uint32_t* cell_first_leaf, const uint32_t* cell_leaf_count, size_t n_cells,
                            const uint32_t* far_offsets, const uint32_t* far_cells);
/* Moments of the LAST evaluation as the far pass used them, before the fp32 rounding: mass_out[n_cells], com_out[n_cells * dim]
 * (centre of mass of a massless cell: zeros).  Either pointer may be NULL.  Synchronises.  NBX_ERR_STATE before the first
 * evaluation with these cells; a plan without cells writes nothing. */
int nbx_leaf_plan_get_cells(nbx_leaf_plan* plan, double* mass_out, double* com_out);
/* Counts, and the device time of the last evaluation's moment and far kernels when that evaluation was timed (kernel_ms != NULL;
 * 0 otherwise); kernel_ms of the evaluation itself keeps meaning the near-field pair kernel.  Any pointer may be NULL. */
int nbx_leaf_plan_cell_info(nbx_leaf_plan* plan, size_t* n_cells, size_t* far_entries, float* moments_ms, float* far_ms);

/* ---- the order of the far field ---------------------------------------------------------------------------------------------
 * NBX_FAR_MONOPOLE (every plan's order until told otherwise): a far cell attracts as one pseudo-body, as described above.
 * NBX_FAR_QUADRUPOLE adds the second-order term of the expansion of the cell's bodies about its centre of mass (the first-order
 * term, the dipole, vanishes there).  The law is m d / r^4 per unit target mass, one power of r steeper than Newton's; d / r^4 is
 * not the gradient of a harmonic function in 3D, so the textbook traceless quadrupole does not apply and the FULL symmetric second
 * moment is used:
 *   moments: Q_ab = sum m_j s_a s_b, s = p_j - com_c, over the bodies of the cell's leaves, fp64 from the fp32 slot values in the
 *       parallel-axis form -- per leaf about the leaf's own centre of mass, per cell sum_l [ Q_l + M_l (c_l - c)(c_l - c)^T ] --
 *       so that nothing cancels; fixed order, no atomics, recomputed in every evaluation like M_c and com_c.  Stored and returned
 *       in the order xx, yy, zz, xy, xz, yz (3D) or xx, yy, xy (2D).
 *   term: with R = com_c - p_i, r^2 = |R|^2, q = Q / M_c, cell c adds to body i's sum
 *           (M_c / r^4) [ R (1 - 2 tr(q) / r^2 + 12 R^T q R / r^4) - 4 q R / r^2 ]
 *       -- the first R in the bracket is the monopole term, the rest the correction; the same formula holds in 2D with 2 x 2 q.
 *       q is fp32 on the device (48 bytes per cell with the pseudo-body in 3D, 32 in 2D).  Sign and G m_i are the law's, as for
 *       the monopole; where the law's rule below its threshold skips or softens the pair with the pseudo-body, the correction of
 *       that pair is dropped.
 *   fallback: a cell with M_c == 0, or one for which any entry of q is not finite in fp32 (masses of mixed sign with M_c near 0),
 *       attracts as its monopole alone.  Masses of mixed sign within a cell are outside what the order's claims cover: the
 *       expansion's error is then not bounded by the cell's size, and a q that is finite in fp32 but enormous (M_c near 0) can
 *       still overflow inside the term; with masses of one sign |q| is bounded by the cell's extent squared and nothing overflows.
 * nbx_leaf_plan_set_far_order: waits for the plan's last evaluation; NBX_ERR_INVALID for a null plan or an unknown order (the plan
 * keeps its order).  May be called before or after nbx_leaf_plan_set_cells or an octree build; the order is the plan's and
 * survives set_cells, rebuild_octree and step_octree.  A plan that stays at NBX_FAR_MONOPOLE allocates nothing for second moments
 * and evaluates bit for bit as before. */
enum { NBX_FAR_MONOPOLE = 0, NBX_FAR_QUADRUPOLE = 1 };
int nbx_leaf_plan_set_far_order(nbx_leaf_plan* plan, int order);
int nbx_leaf_plan_get_far_order(const nbx_leaf_plan* plan, int* order);
/* Central second moments Q (not q) of the LAST evaluation as the far pass used them, before the division by M_c and the fp32
 * rounding: q_out[n_cells][dim (dim + 1) / 2] in the order above (a massless cell: zeros).  Synchronises.  NBX_ERR_STATE on a plan
 * at NBX_FAR_MONOPOLE and before the first evaluation at NBX_FAR_QUADRUPOLE with these cells; a plan without cells writes nothing. */
int nbx_leaf_plan_get_cell_quadrupoles(nbx_leaf_plan* plan, double* q_out);

/* ---- softened Newtonian gravity on a plan ------------------------------------------------------------------------------------
 * NBX_LAW_NEWTON: the attractive Plummer-softened law of nbx_ctx_set_law(NBX_FORCE_LAW_NEWTON), evaluated through the plan -- near
 * lists, far cells at either order, the step loops.  Per unit G m_i a source j adds
 *       m_j d / (r^2 + epsilon^2)^(3/2),   d = p_j - p_i
 * and F_i = +G m_i x the sum (the tree laws' sign).  Every pair counts: a body and itself, or two bodies at one position, give
 * exactly 0 (d = 0, a finite weight); there is no threshold and no special case, so every wave runs the pair loop without a
 * compare.  A far cell is a pseudo-body under the same formula; at NBX_FAR_QUADRUPOLE it adds the exact second-order term of the
 * softened kernel with the same full q = Q / M_c the moment pass writes (rho^2 = r^2 + epsilon^2):
 *       (M_c / rho^3) [ R (1 - (3/2) tr(q) / rho^2 + (15/2) R^T q R / rho^4) - 3 q R / rho^2 ]
 * epsilon is the PLAN's (nbx_leaf_plan_set_softening; 0 until told otherwise): 0 or in [1e-6, 1e15], the context's range;
 * NBX_ERR_INVALID outside it and for a null plan, the plan then keeps its value.  The call waits for the plan's last evaluation;
 * the value survives set_cells, rebuild_octree and step_octree.  The three other laws never read it: their results are bit for
 * bit those of a plan never told.
 * An evaluation (nbx_leaf_plan_forces, _forces_ctx, _step, _step_octree, _time_kernel) under NBX_LAW_NEWTON returns, before anything
 * is launched, NBX_ERR_STATE while epsilon is 0, and NBX_ERR_INVALID when max|m| / epsilon^3 -- the heaviest body's weight at zero
 * distance -- is not a finite, normal fp32 number (the context's rule; the largest mass is what the context recorded at upload, or,
 * for host bodies, found in one pass over the masses about to be copied).  RANGE: the pair terms are fp32; rho^-3 is formed as such in
 * the packed waves of small leaves, so the terms keep fp32's precision for rho = sqrt(r^2 + epsilon^2) < 4.4e12 (rho^-3 a normal fp32
 * number) and lose bits gradually beyond -- distances or softening lengths above that are accepted (the m / epsilon^3 rule is about the
 * masses) but outside what the law's accuracy claims cover; the reference laws' 1 / r^4 meets the same limit at r = 3e9.
 * The context's own law and softening are not consulted:
 * set them as well (nbx_ctx_set_law, nbx_ctx_set_softening) for nbx_ctx_energy or an all-pairs check of the same system. */
int nbx_leaf_plan_set_softening(nbx_leaf_plan* plan, double epsilon);
int nbx_leaf_plan_get_softening(const nbx_leaf_plan* plan, double* epsilon);

/* ---- the octree built on the device ---------------------------------------------------------------
 * A fixed-depth octree (quadtree in 2D) over the bodies RESIDENT in a single-shard context, with the near and far lists of a
 * Barnes-Hut walk with opening angle theta (octree.cpp:129-151's test on grid boxes): the tree, both lists, the plan's layout and
 * its far field are all made on the device, on the context's stream; 64 bytes of counts and the planner's 64-byte summary are
 * all the host reads.  The reference rebuilds its tree in every force call (methods.cpp:377-401); nbx_leaf_plan_rebuild_octree
 * is that rebuild, and nbx_leaf_plan_step_octree a whole Barnes-Hut step loop without the bodies or the tree leaving the GPU.
 * The structure is, word for word, the eight arrays the host builders make (leaves.octree_cells, build_octree_cells<D>):
 * leaves = non-empty cells of the 2^depth grid over the 1 %-padded bounding box, in Morton order; cells = the non-empty nodes
 * of levels 1 .. depth; per leaf a near list (itself first) and a far list (coarse levels first).  0 <= depth <= 10; theta >= 0
 * and finite (theta = 0 accepts nothing: every leaf is on every near list).  The plan is bound to the context's device,
 * dimension and body count and works with every nbx_leaf_plan_* call.
 * NBX_ERR_INVALID: null pointers, a context of several shards or without bodies, depth or theta out of range, a coordinate
 * that is not finite (no plan is made), more than 0xfffffff0 near or far entries.  NBX_ERR_STATE: nothing uploaded yet. */
int nbx_leaf_plan_create_octree(nbx_leaf_plan** out, nbx_ctx* ctx, int depth, double theta);
/* The ADAPTIVE octree: leaves of bounded occupancy, for inputs whose density varies (a Plummer sphere's centre puts thousands of
 * bodies into one cell of any fixed depth).  Root box, finest cells (at max_depth), Morton keys and body order are those of
 * nbx_leaf_plan_create_octree(depth = max_depth).  A node is a key prefix at level L <= max_depth.  The root is split when
 * max_depth >= 1 and (leaf_capacity == 0 or n > leaf_capacity); a node of level L >= 1 exists when it is not empty and its parent
 * is split; an existing node is a leaf at L == max_depth or, for leaf_capacity > 0, when it holds at most leaf_capacity bodies,
 * and is split otherwise.  Leaves in Morton order; cells = the existing nodes of levels 1 .. max_depth, level by level (every
 * leaf is one of them); the walk tests a node against the target leaf's OWN box: accepted when node_side < theta * gap, near
 * list when it is a leaf that is not accepted, opened otherwise -- so for every leaf the bodies of its near leaves and far cells
 * number exactly n.  An unsplit root gives one leaf, its near list itself, and no cells.  leaf_capacity = 0 is
 * nbx_leaf_plan_create_octree(depth = max_depth).  The host builders leaves.adaptive_octree_cells and
 * build_adaptive_octree_cells<D> make the same eight arrays word for word.  Errors as nbx_leaf_plan_create_octree; a negative
 * leaf_capacity is NBX_ERR_INVALID.  Every nbx_leaf_plan_* call works on such a plan; a rebuild keeps all three parameters. */
int nbx_leaf_plan_create_octree_adaptive(nbx_leaf_plan** out, nbx_ctx* ctx, int max_depth, int leaf_capacity, double theta);
/* Builds the structure again, with the same depth and theta, from the context's current positions.  The plan's device blocks
 * are reused where they fit.  NBX_ERR_STATE for a plan not made by nbx_leaf_plan_create_octree.  After a refused rebuild the
 * plan holds no structure (evaluations return NBX_ERR_STATE) until a rebuild succeeds. */
int nbx_leaf_plan_rebuild_octree(nbx_leaf_plan* plan, nbx_ctx* ctx);
/* Lengths of the structure built on the device: leaf_offsets, list_offsets and far_offsets have n_leaves + 1 words, leaf_bodies
 * one per body, list_sources near_entries, the two cell arrays n_cells each, far_cells far_entries.  Any pointer may be NULL.
 * NBX_ERR_STATE on plans not built on the device. */
int nbx_leaf_plan_structure_sizes(const nbx_leaf_plan* plan, size_t* n_leaves, size_t* near_entries, size_t* n_cells, size_t* far_entries);
/* Copies the structure to the host (any pointer may be NULL) and synchronises.  NBX_ERR_STATE on plans not built on the device. */
int nbx_leaf_plan_get_structure(nbx_leaf_plan* plan, uint32_t* leaf_offsets, uint32_t* leaf_bodies, uint32_t* list_offsets, uint32_t* list_sources,
                                uint32_t* cell_first_leaf, uint32_t* cell_leaf_count, uint32_t* far_offsets, uint32_t* far_cells);
/* nsteps x { rebuild when rebuild_every > 0 and step % rebuild_every == 0 (steps count from 0); forces_ctx(NULL, NULL);
 * kick_drift }.  rebuild_every = 0 never rebuilds and equals nbx_leaf_plan_step.  Afterwards the plan holds the last step's
 * sums and the last structure built. */
int nbx_leaf_plan_step_octree(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, double dt, int nsteps, int rebuild_every);

/* ---- kick-drift-kick through a plan -------------------------------------------------------------------------------------------
 * nbx_leaf_plan_kick_drift / _step / _step_octree run the reference helpers' order, kick then drift: first order in dt, and x and v
 * are never at one time level.  The calls below are the synchronised second-order leapfrog through the same sums -- the plan's twin
 * of nbx_ctx_kick_drift2 / nbx_ctx_step_kdk.  They add to the ABI; every call above keeps its bits.
 *
 * nbx_leaf_plan_kick_drift2: nbx_leaf_plan_kick_drift with the kick's and the drift's step apart, from the LAST evaluation's sums:
 *       v += (F / m) dt_kick;  x += v dt_drift;  the fp32 source copy follows x
 * F = +-(G m_i) x the sum as nbx_leaf_plan_kick_drift forms it; dt_kick == dt_drift gives that call's bits; a body in no leaf has
 * F = 0 and drifts with its velocity.  dt_drift == 0 is a PURE KICK: no position is read or written (a velocity that is not finite
 * cannot reach one through inf * 0), the context's bodies have not moved, and the plan's structure, the context's accelerations
 * and its close-set lists stay valid.  Asynchronous on the context's stream.  Refusals are nbx_leaf_plan_kick_drift's:
 * NBX_ERR_INVALID for a null argument or a context of the wrong device, dimension, body count or shard count; NBX_ERR_STATE before
 * the first evaluation and when the last evaluation was not made from `ctx`.
 *
 * nbx_leaf_plan_step_kdk: nsteps steps of
 *       F K(dt/2) D(dt) [ F K(dt) D(dt) ]^(nsteps-1) F K(dt/2)
 * with the structure standing (F = nbx_leaf_plan_forces_ctx(NULL, NULL), K D = nbx_leaf_plan_kick_drift2): adjacent half-kicks are
 * merged into one multiply by dt, as in nbx_ctx_step_kdk, so nsteps steps cost nsteps + 1 evaluations.  The opening evaluation is
 * always made -- a plan does not try to know whether its sums are current; a caller who chains calls and wants to save it spells the
 * sequence out with _forces_ctx and _kick_drift2.  TIME LEVELS: afterwards x and v are BOTH at t0 + nsteps dt, and the plan holds the
 * sums of those final positions, so nbx_leaf_plan_get_forces, _max_accel and (with nbx_leaf_plan_energy) the energies all refer to
 * the state the context holds.  Asynchronous.  nsteps == 0 does nothing.  Refusals, before anything is launched, are
 * nbx_leaf_plan_step's (NBX_LAW_NEWTON: nbx_leaf_plan_set_softening's rules).
 *
 * nbx_leaf_plan_step_octree_kdk: the same sequence with rebuilds.  Evaluation number e = 0 .. nsteps is preceded by
 * nbx_leaf_plan_rebuild_octree when rebuild_every > 0 and e % rebuild_every == 0; the closing half-kick follows an evaluation on
 * the structure standing then, so the inverse map and the sums always belong together.  rebuild_every = 0 never rebuilds and
 * equals nbx_leaf_plan_step_kdk.  Far order and softening survive, as through nbx_leaf_plan_step_octree, whose refusals these are
 * (NBX_ERR_STATE for rebuild_every > 0 on a plan not made by nbx_leaf_plan_create_octree). */
int nbx_leaf_plan_kick_drift2(nbx_leaf_plan* plan, nbx_ctx* ctx, double dt_kick, double dt_drift);
int nbx_leaf_plan_step_kdk(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, double dt, int nsteps);
int nbx_leaf_plan_step_octree_kdk(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, double dt, int nsteps, int rebuild_every);
/* The largest acceleration magnitude of the LAST force evaluation -- what a step size is chosen from -- reduced on the device:
 *       *a_max = max over the bodies that have a slot of  |G| sqrt(sum_k sum_i[k]^2)
 * per unit mass (|F_i| / m_i), fp64, under the G given to that evaluation; bodies in no leaf count as 0; a sum that is not finite
 * makes the result not finite (a NaN orders above infinity) instead of vanishing.  An OBSERVER like the potential calls: it
 * synchronises and changes neither the sums, the record of the last evaluation nor the context.  8 bytes cross PCIe.  A plan never
 * asked allocates nothing for it.  NBX_ERR_INVALID for a null argument; NBX_ERR_STATE before the first evaluation (or after a
 * rebuild without one) and when the context of the last evaluation no longer exists. */
int nbx_leaf_plan_max_accel(nbx_leaf_plan* plan, double* a_max);

/* ---- kick-drift-kick with the step chosen on the device -------------------------------------------------------------------------
 * nbx_leaf_plan_step_kdk_adaptive: the kick-drift-kick loop above with every step's size chosen ON THE DEVICE from the evaluation
 * just made (nbx_leaf_plan_max_accel's value of its sums); nothing is read back to choose it.  The rule, in fp64:
 *       t = t_start; prev = 0; steps = 0
 *       for e = 0, 1, 2, ...:
 *           rebuild the octree when rebuild_every > 0 and e % rebuild_every == 0   (as nbx_leaf_plan_step_octree_kdk)
 *           evaluate (nbx_leaf_plan_forces_ctx(NULL, NULL)); a_max = nbx_leaf_plan_max_accel's value for these sums
 *           if a_max is not finite: status = 1; stop                               (no kick is made with these sums)
 *           if t >= t_end or steps == max_steps:                                   the closing half-kick
 *               v += (F / m) (0.5 prev); record (a_max, 0); stop
 *           dt = choose(a_max);  if dt >= t_end - t: dt = t_end - t, t = t_end  else t = t + dt
 *           v += (F / m) (0.5 prev + 0.5 dt);  x += v dt;  prev = dt;  steps += 1;  record (a_max, dt)
 * choose(a_max): raw = sqrt(accel_length / a_max), +infinity when a_max == 0.  pow2 == 0: min(max(raw, dt_min), dt_max).
 * pow2 == 1: d = dt_max; while (d > raw && 0.5 d >= dt_min) d = 0.5 d -- the halvings are exact, so every dt is dt_max 2^-j.  Only
 * the step that lands on t_end may be shorter than dt_min.
 * The kicks are nbx_leaf_plan_kick_drift2's arithmetic: a caller who replays the recorded dt's with _forces_ctx and
 * _kick_drift2(0.5 prev + 0.5 dt, dt), then the closing _kick_drift2(0.5 prev, 0), gets the same bits.  A closing kick with
 * prev == 0 is not applied, and no kick is applied once the loop has stopped.
 * TIME LEVELS: afterwards x and v are BOTH at the clock's t and the plan holds the sums of the final positions -- unless
 * status == 1: then the loop stopped before the kick of the evaluation whose a_max was not finite, x is at t and v is HALF A STEP
 * (0.5 dt_last) BEHIND it.  Far order and softening survive; the potential calls remain observers; max_steps == 0 does nothing.
 * With rebuild_every == 0 the call is asynchronous and reads nothing back: the host cannot know when t_end is reached, so it queues
 * evaluations up to number max_steps; those behind the stop find the positions unmoved, give the same sums, record nothing and kick
 * nothing.  (The loop stops queueing early once a copy it makes anyway has shown it the stop; the results are the same.)
 * Refusals, before anything is launched.  NBX_ERR_INVALID: a null argument, an unknown law, a control outside the ranges given
 * with its fields, reserved != 0, max_steps < 0 or > 1 << 20, rebuild_every < 0 (all of these need no device), the wrong context.
 * NBX_ERR_STATE: rebuild_every > 0 on a plan not made by nbx_leaf_plan_create_octree; NBX_LAW_NEWTON while the softening is 0.
 *
 * nbx_leaf_plan_get_step_clock: where the last adaptive call left the device's clock; synchronises.  NBX_ERR_STATE before the
 * first adaptive call on the plan.  evaluations counts those the rule above acted on (the one that stopped it included).
 * nbx_leaf_plan_get_step_history: the (a_max, dt) pairs recorded by the last adaptive call, oldest first: *count is how many there
 * are, and min(capacity, *count) of them are written (either array may be null).  The closing evaluation's entry has dt = 0. */
typedef struct nbx_step_control {
    double accel_length;    /* c > 0, finite: dt_raw = sqrt(c / a_max); c = eta^2 * epsilon is the usual choice */
    double dt_min, dt_max;  /* 0 < dt_min <= dt_max, finite */
    double t_start, t_end;  /* t_start finite; t_end finite or +infinity, not NaN */
    int    pow2;            /* 0: dt = clamp(dt_raw, dt_min, dt_max); 1: dt = dt_max / 2^j (rule above) */
    int    reserved;        /* must be 0 */
} nbx_step_control;
typedef struct nbx_step_clock {
    double t, dt_last, a_max_last;
    uint32_t steps, evaluations;
    int finished;           /* 1: t reached t_end */
    int status;             /* 0 ok; 1: an a_max was not finite, the loop stopped before kicking with it */
} nbx_step_clock;
int nbx_leaf_plan_step_kdk_adaptive(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, const nbx_step_control* control, int max_steps,
                                    int rebuild_every);
int nbx_leaf_plan_get_step_clock(nbx_leaf_plan* plan, nbx_step_clock* clock);
int nbx_leaf_plan_get_step_history(nbx_leaf_plan* plan, double* a_max_out, double* dt_out, size_t capacity, size_t* count);

/* ---- the potential through a plan -------------------------------------------------------------------------------------------
 * What the plan's sums are the gradient of, through the same near lists and far cells, in O(list length) like the forces.  Per unit
 * G m_i, body i of target leaf t has
 *       phi_i = sum over bodies j != i of the leaves on t's near list of  m_j w(r_ij)
 *             + sum over the cells c on t's far list of                   Phi_c(R),   R = com_c - p_i
 * with the law's pair potential w:
 *       NBX_LAW_NEWTON      w = 1 / rho, rho^2 = r^2 + epsilon^2; the body itself is left out by IDENTITY (its own slot), so two
 *                           different bodies at one position count m_j / epsilon
 *       NBX_LAW_BRUTE       w = 1 / (2 r^2); pairs with r^2 < 1e-10 are left out (the law's own skip)
 *       NBX_LAW_TREE_LEAF   w = 1 / (2 r^2); pairs with r^2 < 1e-9 are left out
 *       NBX_LAW_FMM_P2P     NBX_ERR_INVALID: its smoothed magnitude with unsmoothed direction below 1e-10 is no gradient
 * A far cell with q = Q / M_c (the record the moment pass writes) and t = tr q adds, at NBX_FAR_MONOPOLE / NBX_FAR_QUADRUPOLE,
 *       NEWTON      M_c / rho         (M_c / rho)     [ 1 - t / (2 rho^2) + (3/2) R^T q R / rho^4 ]
 *       reference   M_c / (2 r^2)     (M_c / (2 r^2)) [ 1 - t / r^2       + 4     R^T q R / r^4   ]
 * (0 where the law skips the pair with the pseudo-body; a massless cell adds 0; a cell whose q record is the all-zero fallback adds
 * its monopole alone).  Totals: U = s (G / 2) sum_i m_i phi_i with s = +1 for NBX_LAW_BRUTE (on complete lists nbx_ctx_energy's
 * potential) and -1 for the two others (NEWTON: -sum_{i<j} G m_i m_j / rho); K = sum_i m_i |v_i|^2 / 2 from the context's fp64 state.
 * A body in no leaf has phi_i = 0 and still counts in K.  The terms are fp32 like every pair term, the sums fp64 in a fixed order.
 *
 * A potential call is an OBSERVER.  It leaves untouched the slot sums of the last force evaluation, that evaluation's law, sign and
 * masses, and the context's bodies: nbx_leaf_plan_get_forces, _kick_drift, _step and _step_octree afterwards give the bits they would
 * have given without it.  It does gather the source pairs again and recompute the cells' moments: nbx_leaf_plan_get_cells,
 * _get_cell_quadrupoles and _time_kernel afterwards refer to the positions the potential call saw.  On a plan built on the device
 * the structure is the one of the last (re)build; the call does not rebuild.  The far order and the softening length are the plan's.
 * A plan never asked for a potential allocates nothing for it.  Every call synchronises.
 * Refused before anything is launched: NBX_ERR_INVALID for a null plan / ctx / phi_out, an unknown law or NBX_LAW_FMM_P2P, a refused
 * body stride, a context of the wrong device, dimension, body count or shard count, and max|m| / epsilon^3 outside fp32's normal
 * range (nbx_leaf_plan_set_softening's rule); NBX_ERR_STATE for NBX_LAW_NEWTON while epsilon is 0, a context with nothing uploaded,
 * and a plan whose last octree build was refused.  There is no CPU fallback. */
/* host bodies in, per-body potentials out: phi_out[n_bodies], per unit G m_i; the twin of nbx_leaf_plan_forces */
int nbx_leaf_plan_potentials(nbx_leaf_plan* plan, const void* bodies, size_t body_stride_bytes, int law, double* phi_out);
/* resident bodies: the context's positions as they stand now, the moment pass (if the plan has cells), near + far potential,
 * reduction.  Either out pointer may be NULL. */
int nbx_leaf_plan_energy(nbx_leaf_plan* plan, nbx_ctx* ctx, int law, double G, double* kinetic, double* potential);
/* phi of the last nbx_leaf_plan_energy / _potentials call, n_bodies doubles; NBX_ERR_STATE before the first */
int nbx_leaf_plan_get_potentials(nbx_leaf_plan* plan, double* phi_out);

/* ---- device-resident context ------------------------------------------------------------------
 * A context owns the targets of ONE shard of an N-body system on ONE device and a full-length
 * fp32 copy of all N sources.  n_shards = 1, shard = 0 is the single-GPU case.  With n_shards = G
 * the bodies are split into G contiguous shards of shard_len = ceil(N/G) bodies (the last one
 * short); rank g creates a context with shard = g and exchanges fp32 positions with the others
 * once per step (RCCL all-gather of the buffer described by nbx_ctx_gather_layout).
 */
int nbx_ctx_create(nbx_ctx** out, int device, int dim, size_t n_total, int n_shards, int shard);
int nbx_ctx_destroy(nbx_ctx* ctx);

/* Use a caller-owned HIP stream (hipStream_t as void*) for every launch and copy of this context;
 * NULL restores the context's own stream.  Lets a torch.cuda.Stream order the kernels. */
int nbx_ctx_set_stream(nbx_ctx* ctx, void* hip_stream);

/* Use caller-owned device memory for the two all-gather buffers (see nbx_ctx_gather_layout for the
 * required sizes).  Must be called before nbx_ctx_upload_bodies.  This is how the one-process-per-
 * GPU host layer hands torch-allocated tensors to RCCL and to the kernels without a copy. */
int nbx_ctx_set_gather_buffers(nbx_ctx* ctx, void* pos_all_f32, void* mass_all_f32);

/* Layout of the exchange buffers:
 *   pos_all : float[n_shards][dim][shard_pad]   -- chunk g = shard g's x[], y[], (z[]) arrays
 *   mass_all: float[n_shards][shard_pad]
 * shard_len = bodies per shard, shard_pad = shard_len rounded up to a multiple of 4096 bodies; pad
 * entries are massless bodies at the origin (they contribute exactly zero).
 * Any out pointer may be NULL. */
int nbx_ctx_gather_layout(const nbx_ctx* ctx, size_t* shard_len, size_t* shard_pad,
                          void** pos_all_f32, void** mass_all_f32);

/* Upload ALL n_total bodies (Body<dim> array as above).  Fills the fp32 source copy for every
 * shard and the fp64 position/velocity/mass state of this context's own shard. */
int nbx_ctx_upload_bodies(nbx_ctx* ctx, const void* bodies, size_t body_stride_bytes);

/* The same upload for a sharded context that moves only ITS OWN bodies over the host link (one process per GPU: every rank
 * uploading the whole array costs G copies of it):
 *   1. nbx_ctx_upload_shard: shard_bodies = the shard_len-or-fewer bodies this context owns (Body<dim> array); packs the own
 *      chunk of the exchange buffers and the fp64 state; returns the largest |mass| and |coordinate| of the shard;
 *   2. the caller fills the OTHER chunks of pos_all / mass_all device to device (one all-gather of each; layout above) and
 *      combines the two maxima over all ranks;
 *   3. nbx_ctx_upload_finish with the combined maxima: the fast path's preconditions are decided from them (they are properties
 *      of all bodies), and -- for small-coordinate systems -- the close-set probe runs against every chunk.
 * nbx_ctx_upload_bodies = the three steps on the whole array in one call. */
int nbx_ctx_upload_shard(nbx_ctx* ctx, const void* shard_bodies, size_t body_stride_bytes, double* max_abs_mass, double* max_abs_coord);
int nbx_ctx_upload_finish(nbx_ctx* ctx, double max_abs_mass_all, double max_abs_coord_all);

/* Accelerations of this shard's targets: a_i = sum_j m_j (p_j - p_i)/r^4 over the selected sources
 * (the reference force without the -(G m_i) factor).  which: 0 = all shards' sources,
 * 1 = only this shard's own chunk (needs no remote data), 2 = every other shard's chunk, added to
 * what a preceding which=1 call produced.  Asynchronous on the context's stream. */
enum { NBX_SRC_ALL = 0, NBX_SRC_LOCAL = 1, NBX_SRC_REMOTE = 2 };
int nbx_ctx_compute_accel(nbx_ctx* ctx, int which);

/* Fused kick + drift for this shard (methods.cpp:425-438 then :440-450, fp64):
 *   F = -(G m) a;  v += (F / m) * dt;  x += v * dt;
 * and refresh of this shard's fp32 chunk of pos_all.  Asynchronous on the context's stream. */
int nbx_ctx_kick_drift(nbx_ctx* ctx, double G, double dt);
/* The same kernel with separate steps for the two helpers:  v += (F / m) * dt_kick;  x += v * dt_drift.
 * dt_drift = 0 is a pure kick (update_body_velocities alone): positions, accelerations and close-set lists stay valid. */
int nbx_ctx_kick_drift2(nbx_ctx* ctx, double G, double dt_kick, double dt_drift);

/* nsteps x { compute_accel(ALL); kick_drift } -- single-shard contexts only (n_shards == 1).  From 4 steps
 * on, one step is captured into a hipGraph and replayed (launch-bound regime at small N); nbx_ctx_kernel_time
 * then reports those steps by their whole-step time (one event pair around the replay sequence).
 * NBODY_HIP_NO_GRAPHS=1 disables the capture. */
int nbx_ctx_step(nbx_ctx* ctx, double G, double dt, int nsteps);
/* EXTENSION: the same two helpers composed as a synchronised kick-drift-kick leapfrog (second order in dt):
 *   v += (F/m) dt/2;  x += v dt;  F = forces(x);  v += (F/m) dt/2      per step,
 * with adjacent half-kicks merged: nsteps + 1 force evaluations for nsteps steps.  Single-shard contexts only; the
 * sharded form is nbx_node_step_kdk.  (nbx_ctx_step is the reference helpers' plain order, kick then drift: first order.) */
int nbx_ctx_step_kdk(nbx_ctx* ctx, double G, double dt, int nsteps);

/* EXTENSION: kick-drift-kick with the step chosen on the device, for the all-pairs context.
 * nbx_ctx_max_accel: *a_max = max over this shard's real bodies l < count of |G| sqrt(sum_k A_k[l]^2), fp64, where A_k[l] is the
 * fp64 sum of the context's partial sums in plane order -- after the mixed mode's fold and the close-set scatter, the number the
 * next kick would use.  Pads never count; an empty shard gives 0; a sum that is not finite makes the result not finite.  An observer:
 * it synchronises the stream, changes no state, and 8 bytes return.  On a multi-shard context it is this shard's maximum once this
 * shard's sums are complete (after LOCAL + REMOTE); the caller takes the maximum over the ranks.  NBX_ERR_INVALID for a null
 * argument, NBX_ERR_STATE without accelerations on the device.
 * nbx_ctx_step_kdk_adaptive: nbx_ctx_step_kdk with every step's size chosen ON THE DEVICE from the evaluation just made.  It follows
 * the rule written above for nbx_leaf_plan_step_kdk_adaptive word for word (choose, the landing on t_end, the closing half-kick,
 * status == 1, the TIME LEVELS) with rebuild_every = 0, where "evaluate" is nbx_ctx_compute_accel(NBX_SRC_ALL), a_max is
 * nbx_ctx_max_accel's value and the kicks are nbx_ctx_kick_drift2's arithmetic: replaying the recorded dt's with
 * nbx_ctx_compute_accel and nbx_ctx_kick_drift2(0.5 prev + 0.5 dt, dt), then the closing nbx_ctx_kick_drift2(0.5 prev, 0), gives the
 * same bits.  Every law, softening, dimension, precision mode and kernel variant of nbx_ctx_compute_accel; single-shard contexts
 * only.  Asynchronous on the context's stream up to the window below.  Afterwards the context holds the accelerations of the final
 * positions, like nbx_ctx_step_kdk; the opening evaluation is skipped when the context already holds valid ones (its reduction
 * never is).  max_steps == 0 does nothing and leaves no clock.
 * THE WINDOW: the host cannot know when the loop stops, and an evaluation queued behind the stop changes nothing but costs a whole
 * all-pairs pass.  The loop therefore queues evaluation e >= W only after a 4-byte copy made behind evaluation e - W has shown that
 * the loop had not stopped there: at most W - 1 evaluations are wasted, and the results do not depend on W.  The environment
 * variable NBODY_HIP_STEP_WINDOW in [1, 64], read when the context is created, overrides the library's W.
 * Refusals, before anything is launched.  NBX_ERR_INVALID (all of these need no device): a null control, a control outside the
 * ranges given with its fields, reserved != 0, max_steps < 0 or > 1 << 20; a null context.  NBX_ERR_STATE: nothing uploaded; a
 * context with n_shards != 1; and whatever nbx_ctx_compute_accel refuses (NBX_FORCE_LAW_NEWTON without a softening length, ...).
 * nbx_ctx_get_step_clock / nbx_ctx_get_step_history: as nbx_leaf_plan_get_step_clock / _get_step_history, for the context's last
 * adaptive call; NBX_ERR_STATE before the first one. */
int nbx_ctx_max_accel(nbx_ctx* ctx, double G, double* a_max);
int nbx_ctx_step_kdk_adaptive(nbx_ctx* ctx, double G, const nbx_step_control* control, int max_steps);
int nbx_ctx_get_step_clock(nbx_ctx* ctx, nbx_step_clock* clock);
int nbx_ctx_get_step_history(nbx_ctx* ctx, double* a_max_out, double* dt_out, size_t capacity, size_t* count);

/* EXTENSION: forces on a list of targets.  Single-shard contexts with a softening length > 0, under either law.
 * nbx_ctx_compute_accel_active: for every r < n_targets the sum over ALL n_total bodies, at the positions the context holds now, of
 * the law's pair term on body targets[r] -- what nbx_ctx_compute_accel computes for that body, in the same fp32 pair arithmetic
 * (a tile of 256 sources summed in fp32, the tiles in fp64), for O(n_targets * n_total) work.  The list may be in any order and may
 * repeat an index: each row is evaluated by itself.  n_targets == 0 is legal.  The list is copied to the device (the call returns
 * when the copy has; the kernels run asynchronously); on the device the list's LENGTH is a word in memory too, and everything about
 * the launch that depends on it is decided there -- the block-step loop below fills list and length without the host.  Two builds
 * are queued, one target per lane for a short list and eight for a long one; each returns at once unless the length is on its side
 * of a threshold (NBODY_HIP_ACTIVE_LONG_LIST in [1, 2^31], read when the context is created, overrides the library's).  The two
 * agree to rounding, not bit for bit; the same build of the same list gives the same bits (no floating-point atomics).
 * An OBSERVER: the context's accelerations (nbx_ctx_get_forces, _kick_drift), bodies and step clocks are untouched.
 * nbx_ctx_get_forces_active: row r of forces_out (n_targets x Vector<dim>, list order) = the force on body targets[r], with
 * nbx_ctx_get_forces' sign and G m_i scaling.  Synchronises the stream.
 * Refusals, before anything is launched.  NBX_ERR_INVALID (these need no device): a null context; a null list with n_targets > 0;
 * an index >= n_total; a null forces_out with rows to write.  NBX_ERR_STATE: nothing uploaded; n_shards != 1; softening 0;
 * nbx_ctx_get_forces_active without a preceding nbx_ctx_compute_accel_active (an upload or a block-step call ends its validity).
 * The m / eps^p range rule of nbx_ctx_compute_accel applies (NBX_ERR_INVALID). */
int nbx_ctx_compute_accel_active(nbx_ctx* ctx, const uint32_t* targets, size_t n_targets);
int nbx_ctx_get_forces_active(nbx_ctx* ctx, double G, double* forces_out);

/* EXTENSION: kick-drift-kick with BLOCK time steps.  Body i has its own step dt_max 2^-level_i; every body drifts on the smallest step
 * present (O(N)); forces are computed, through nbx_ctx_compute_accel_active's kernels, only for the bodies whose own step ends
 * (O(n_active N)).  Lists, levels, the clock and every decision stay on the device.  The rule, in fp64 without contraction:
 *       tick = dt_max 2^-L;  level l has the step dt_l = dt_max 2^-l = 2^(L-l) ticks;  T_end = n_blocks 2^L
 *       want(a): raw = sqrt(accel_length / a), +infinity when a == 0;  w = 0; d = dt_max; while (d > raw && w < L) { d = 0.5 d; ++w; }
 *       T = 0; all bodies active
 *       for every evaluation:
 *           sums of the active bodies (ascending body index) from ALL bodies' current positions;  a_i = |G| |A_i|
 *           any a_i not finite: status = 1; stop                                  (nobody is kicked with these sums)
 *           for active i, old = level_i, w = want(a_i):
 *               first evaluation of the call:  new = w;  kick = 0.5 dt_new
 *               later:  new = w        if w > old
 *                       new = old - 1  if w < old and old > 0 and T % 2^(L-old+1) == 0        (one level up, where the longer step is aligned)
 *                       new = old      otherwise;   at T == T_end: new = old
 *                       kick = 0.5 dt_old + (T == T_end ? 0 : 0.5 dt_new)
 *               v_i += (F_i / m_i) kick                                           (nbx_ctx_kick_drift2's arithmetic and sign)
 *               level_i = new
 *           record (n_active, dn);  pair_terms += n_active n_total                 (dn: the ticks of the drift that follows, 0 when none does)
 *           T == T_end: finished = 1; stop
 *           substeps == max_substeps: status = 2; stop
 *           dn = 2^(L - deepest level present among ALL bodies)
 *           x += v (dn tick) for ALL bodies, the fp32 positions refreshed;  T += dn;  t = t_start + T tick;  substeps += 1
 *           active = { i : T % 2^(L - level_i) == 0 }
 * T is always a multiple of every present step, so every body is active at T_end and afterwards x and v are at one time.  levels = 0
 * is nbx_ctx_step_kdk(dt_max, n_blocks) through the list kernels.  A later call starts from fresh levels.
 * TIME LEVELS: after status == 2 (max_substeps reached before T_end) the bodies are NOT at one time: x is at t, body i's velocity is
 * half its own step behind the end of its last step, and a later call does not resume this one.  After status == 1 the loop stopped
 * before the kick of the evaluation whose sums were not finite.  Afterwards the context holds no valid accelerations.
 * The call is asynchronous and reads nothing back to choose anything: it queues evaluations up to number max_substeps + 1; behind the
 * stop every kernel returns at once.  (It stops queueing early once a 4-byte look it makes anyway has shown the stop --
 * NBODY_HIP_STEP_WINDOW, as for nbx_ctx_step_kdk_adaptive; the results do not depend on it.)
 * Refusals, before anything is launched.  NBX_ERR_INVALID (all of these need no device): a null control, a field outside the range
 * given with it, reserved != 0, n_blocks < 0, max_substeps < 0 or > 1 << 20; a null context.  NBX_ERR_STATE: nothing uploaded, a
 * context with n_shards != 1, softening 0.  n_blocks == 0 does nothing and leaves no clock.
 * nbx_ctx_get_block_clock: where the last block-step call left the device's clock; synchronises.  deepest_level is the deepest level
 * any body held during the call.  nbx_ctx_get_block_history: the (n_active, dn) pairs recorded, oldest first: *count is how many there
 * are, min(capacity, *count) are written (either array may be null).  nbx_ctx_get_block_levels: the bodies' levels as the call left
 * them (count entries).  All three: NBX_ERR_STATE before the first block-step call. */
typedef struct nbx_block_control {
    double accel_length;   /* c > 0, finite */
    double dt_max;         /* > 0, finite */
    double t_start;        /* finite */
    int    levels;         /* L in [0, 20] */
    int    reserved;       /* must be 0 */
} nbx_block_control;
typedef struct nbx_block_clock {
    double t;
    uint64_t ticks;        /* T */
    uint64_t pair_terms;   /* sum over the evaluations of n_active * n_total */
    uint32_t substeps, evaluations;
    int deepest_level;
    int finished;          /* 1: T reached T_end */
    int status;            /* 0 ok; 1: an acceleration was not finite; 2: max_substeps reached before the end */
} nbx_block_clock;
int nbx_ctx_step_kdk_block(nbx_ctx* ctx, double G, const nbx_block_control* control, int n_blocks, int max_substeps);
int nbx_ctx_get_block_clock(nbx_ctx* ctx, nbx_block_clock* clock);
int nbx_ctx_get_block_history(nbx_ctx* ctx, uint32_t* n_active_out, uint32_t* ticks_out, size_t capacity, size_t* count);
int nbx_ctx_get_block_levels(nbx_ctx* ctx, int32_t* levels_out);

/* EXTENSION: accelerations and their time derivatives (jerks) of a list of targets -- nbx_ctx_compute_accel_active's twin for
 * fourth-order schemes.  For every r < n_targets, over ALL n_total bodies at the positions AND velocities the context holds now:
 *       A_r = sum_j m_j w d,     J_r = sum_j m_j w [ dv - p (d.dv) / rho^2 d ],
 *       d = p_j - p_r,  dv = v_j - v_r,  rho^2 = r^2 + eps^2,  w = rho^-p,  p = 4 (the softened reference law) or 3 (NBX_FORCE_LAW_NEWTON):
 * J is the exact time derivative of A along straight paths.  The pair arithmetic, the summation (fp32 over a tile of 256 sources, the
 * tiles in fp64, no floating-point atomics), the two builds -- one target per lane for a short list, four for a long one -- and
 * NBODY_HIP_ACTIVE_LONG_LIST are nbx_ctx_compute_accel_active's; the sources' velocities are the fp32 roundings of the context's,
 * refreshed by the call.  A coincident pair with different velocities contributes the finite term m dv / eps^p.  An OBSERVER: bodies,
 * accelerations and clocks are untouched.  (It shares the device's target list with nbx_ctx_compute_accel_active: each of the two
 * compute calls ends the validity of the other's results.)
 * nbx_ctx_get_accel_jerk_active: row r of accel_out / jerk_out (n_targets x Vector<dim>, list order; either may be null) =
 * -(G' A_r) and -(G' J_r), G' = G under the reference law and -G under NBX_FORCE_LAW_NEWTON: the acceleration F / m that the
 * context's kicks apply to body targets[r] and its time derivative -- accelerations, not forces, so that a massless tracer keeps its
 * row.  Synchronises the stream.
 * Refusals: nbx_ctx_compute_accel_active's, word for word; nbx_ctx_get_accel_jerk_active is NBX_ERR_STATE without a preceding
 * nbx_ctx_compute_accel_jerk_active (an upload, the other compute call or a block-step call ends its validity). */
int nbx_ctx_compute_accel_jerk_active(nbx_ctx* ctx, const uint32_t* targets, size_t n_targets);
int nbx_ctx_get_accel_jerk_active(nbx_ctx* ctx, double G, double* accel_out, double* jerk_out);

/* EXTENSION: the fourth-order HERMITE scheme with block time steps.  Body i has its own step dt_max 2^-level_i, its own time t_i and
 * (x, v, a, j) at that time; ALL bodies are predicted to the current time (O(N)); accelerations and jerks are computed, through
 * nbx_ctx_compute_accel_jerk_active's kernels, only for the bodies whose own step ends (O(n_active N)), and those are corrected.
 * tick, dt_l, T_end, want(raw) and the level rule are nbx_ctx_step_kdk_block's.  The rule, in fp64 without contraction
 * (a = -(G' A), j = -(G' J) as above; |.| the Euclidean length, squares added in component order):
 *       evaluation 0 (T = 0, all bodies): (a, j) from x, v.  Any component not finite: status = 1; stop.
 *           raw_i = eta_start |a_i| / |j_i|   (+infinity when |j_i| == 0);  level_i = want(raw_i);  t_i = 0
 *       after every evaluation: record (n_active, dn);  pair_terms += n_active n_total
 *           T == T_end: finished = 1; stop.     substeps == max_substeps: status = 2; stop.
 *           dn = 2^(L - deepest level present);  T += dn;  t = t_start + T tick;  substeps += 1
 *       predict ALL bodies, h = (T - t_i) tick:
 *           xp = x + v h + a h^2/2 + j h^3/6,   vp = v + a h + j h^2/2
 *           the fp32 positions and velocities (the kernels' sources) are written from xp, vp; x, v themselves stay
 *       active = { i : T % 2^(L - level_i) == 0 };  (a1, j1) of the active bodies from the predicted fp32 positions and velocities
 *       any component not finite: status = 1; stop; nobody is corrected
 *       correct the active bodies, h = dt_level_i:
 *           v1 = v + (h/2)(a + a1) + (h^2/12)(j - j1)
 *           x1 = x + (h/2)(v + v1) + (h^2/12)(a - a1)
 *           a2 = (-6 (a - a1) - h (4 j + 2 j1)) / h^2
 *           a3 = (12 (a - a1) + 6 h (j + j1)) / h^3
 *           a2e = a2 + h a3
 *           raw = sqrt( eta (|a1| |a2e| + |j1|^2) / (|j1| |a3| + |a2e|^2) )       (+infinity when the denominator is 0)
 *           w = want(raw):  new = w if w > old;  old - 1 if w < old and old > 0 and T % 2^(L-old+1) == 0;  old otherwise;  at T_end: old
 *           (x, v, a, j, t_i, level_i) = (x1, v1, a1, j1, T, new);  the fp32 position and velocity of i are written from x1, v1
 * Every body is active at T_end, so afterwards the context's bodies and its fp32 sources are the corrected state at ONE time:
 * nbx_ctx_energy and a download see it.  levels = 0 is the shared-step Hermite scheme with dt_max.  A later call starts afresh
 * (evaluation 0, fresh levels).
 * TIME LEVELS: after status == 2 (max_substeps reached before T_end) the bodies are NOT at one time: body i's x and v are at its own
 * t_i, the end of its last own step (the fp32 sources are put back to their roundings), and a later call does not resume this one.
 * After status == 1 the loop stopped before anybody
 * was corrected with the sums that were not finite.  Afterwards the context holds no valid accelerations (nbx_ctx_get_forces is
 * refused).
 * The call is asynchronous and reads nothing back to choose anything; it stops queueing through nbx_ctx_step_kdk_block's window of
 * 4-byte looks (NBODY_HIP_STEP_WINDOW), and the results do not depend on it.
 * nbx_ctx_get_block_clock / _history / _levels report the last block-step call of EITHER kind.  A Hermite call counts evaluation 0:
 * evaluations == substeps + 1 when it finishes or meets the cap.
 * Refusals, before anything is launched.  NBX_ERR_INVALID (all of these need no device): a null control, a field outside the range
 * given with it, reserved != 0, n_blocks < 0, max_substeps < 0 or > 1 << 20; a null context.  NBX_ERR_STATE: nothing uploaded, a
 * context with n_shards != 1, softening 0.  n_blocks == 0 does nothing and leaves no clock. */
typedef struct nbx_hermite_control {
    double eta;            /* accuracy parameter of Aarseth's criterion: > 0, finite */
    double eta_start;      /* the same for the first step, chosen from |a| / |j| alone: > 0, finite */
    double dt_max;         /* > 0, finite */
    double t_start;        /* finite */
    int    levels;         /* L in [0, 20] */
    int    reserved;       /* must be 0 */
} nbx_hermite_control;
int nbx_ctx_step_hermite_block(nbx_ctx* ctx, double G, const nbx_hermite_control* control, int n_blocks, int max_substeps);

/* Forces of this shard's targets as Vector<dim>[count] doubles: F_i = -(G m_i) a_i.  count = this shard's bodies: shard_len, or
 * fewer -- possibly none -- for the last shards (a shard g with g * shard_len >= n_total is empty); exactly count rows are written.
 * Synchronises the stream. */
int nbx_ctx_get_forces(nbx_ctx* ctx, double G, double* forces_out);
/* The reference's accuracy metric (utils.h:170-219, ACCURACY_PCT_THRESHOLD 1 %, ACCURACY_FORCE_THRESHOLD 1e-20)
 * evaluated on the device against reference_forces (host, Vector<dim>[count] of this shard: count rows are read): percent of
 * bodies whose every force component is within 1 % (absolute 1e-9 where |ref| < 1e-20).  An empty shard (count = 0) reads
 * nothing and reports 0.0, as the reference's compute_accuracy does for no bodies.  The device forces are
 * never copied back; 4 bytes return.  Synchronises the stream. */
int nbx_ctx_accuracy(nbx_ctx* ctx, double G, const double* reference_forces, double* percent);
/* Raw fp32 accelerations, SoA float[dim][count] (component k of target l at accel_out[k * count + l]; count as for
 * nbx_ctx_get_forces -- the last shard's rows are packed, not spaced shard_len apart): the fp32 rounding of the fp64 sum of the
 * slices' partial sums that nbx_ctx_get_forces scales by -(G m).  Synchronises the stream. */
int nbx_ctx_get_accel(nbx_ctx* ctx, float* accel_out);
/* Write this shard's positions and velocities (fp64 state) back into the caller's full-length
 * Body<dim> array (only entries [shard*shard_len, ...) are touched).  Synchronises the stream. */
int nbx_ctx_download_bodies(nbx_ctx* ctx, void* bodies, size_t body_stride_bytes);

/* Energy diagnostic (for energy-drift checks; the reference has none -- SURVEY 5): this shard's share of
 *   kinetic   = sum_i m_i |v_i|^2 / 2                       (fp64 state)
 *   potential = sum_i (G m_i / 4) sum_{j != i} m_j / r_ij^2   (fp32 pair terms, fp64 sums, pairs with
 *               r^2 < 1e-10 skipped) -- summed over all shards this is U = sum_{i<j} G m_i m_j / (2 r^2),
 * the potential whose gradient is the reference's force law (methods.cpp:21-37), so kinetic + potential is
 * what a symplectic kick/drift conserves.  Uses the positions currently in the exchange buffer for the
 * sources.  One O(N^2/G) kernel; synchronises the stream. */
int nbx_ctx_energy(nbx_ctx* ctx, double G, double* kinetic, double* potential);

int nbx_ctx_synchronize(nbx_ctx* ctx);

/* Tuning knobs.  source_splits: number of slices the source loop is cut into (0 = automatic, else a
 * lower bound in [1,256]; more workgroups for small shards; partial sums are combined in a fixed
 * order).  variant: force-kernel variant id in [0, nbx_num_variants()), -1 = library default (see
 * DESIGN.md for the table).  "fast" variants drop the per-pair r^2 guard, find the targets that own a
 * pair closer than 1e-3 exactly (candidates = a coordinate below 16384 in magnitude, checked against each
 * other once per position update) and evaluate those with the guarded kernel inside the same launch, so the
 * result keeps the reference's skip semantics; small-coordinate systems (more than 1/8 of the shard in the candidate set)
 * find their close pairs through sorted cells instead; when a mass exceeds 1e10, or more than 1/8 of the shard really
 * owns a pair closer than 1e-3, the library substitutes the guarded default. */
int nbx_ctx_set_tuning(nbx_ctx* ctx, int source_splits, int variant);
/* How the fast path currently keeps the reference's r^2 < 1e-10 skip rule (diagnostic):
 *   NBX_CLOSE_CANDIDATE_PAIRS  candidate targets x candidate sources (few bodies have a coordinate below 16384)
 *   NBX_CLOSE_SORTED_CELLS     most bodies are candidates: close pairs found through sorted cells
 *   NBX_CLOSE_GUARDED_KERNEL   the per-pair guarded kernel runs instead (mass above 1e10, > 1/8 of the shard owning a close
 *                              pair, or an exact variant selected)
 *   NBX_CLOSE_NONE             softened law: nothing to guard
 * Decided at upload and re-evaluated during long runs from an asynchronous read-back of the device counters every 16
 * steps (never a wait) -- also inside one long nbx_ctx_step call, whose graph replays go out in blocks of 16 steps (the look takes effect
 * within the call only while the device keeps up with the host: at large N the host has queued every block before the first
 * copy lands, and the next call acts on it; a change of mode inside the call drains the stream before the step is re-captured).  candidates_seen / bad_seen: the most recent counts the host has seen (0 before the first). */
enum { NBX_CLOSE_CANDIDATE_PAIRS = 0, NBX_CLOSE_SORTED_CELLS = 1, NBX_CLOSE_GUARDED_KERNEL = 2, NBX_CLOSE_NONE = 3 };
int nbx_ctx_close_set_mode(nbx_ctx* ctx, int* mode, unsigned* candidates_seen, unsigned* bad_seen);

/* EXTENSION (not in the reference: its brute force is unsoftened): Plummer softening of the pair law,
 *   a_i = sum_{j != i} m_j (p_j - p_i) / (r^2 + epsilon^2)^2 ,   U = sum_{i<j} G m_i m_j / (2 (r^2 + epsilon^2)),
 * every pair counted (no r^2 < 1e-10 skip; a body never acts on itself).  epsilon = 0 (default) is the reference law.
 * Same kernel, same speed: epsilon^2 replaces the fast kernel's r^2 bias and no close-set bookkeeping is needed.
 * epsilon must be 0 or in [1e-6, 1e15], and max|m| / epsilon^4 (Newtonian law: / epsilon^3) must be a finite, normal fp32
 * number -- neither overflow nor underflow to an all-zero field (checked at the next force evaluation: NBX_ERR_INVALID; with
 * the reference's masses up to 1e8 that is epsilon <= ~3e9).  Applies to compute_accel / step / energy of this context. */
int nbx_ctx_set_softening(nbx_ctx* ctx, double epsilon);
/* EXTENSION (SURVEY 5/7 `--law {reference,newton}`; the reference has one law): NBX_FORCE_LAW_REFERENCE (default) is the
 * reference's repulsive m_j d / r^4 form; NBX_FORCE_LAW_NEWTON is the attractive, Plummer-softened Newtonian law
 *   F_i = +G m_i sum_{j != i} m_j (p_j - p_i) / (r^2 + epsilon^2)^(3/2),   U = -sum_{i<j} G m_i m_j / sqrt(r^2 + epsilon^2),
 * which needs a softening length > 0 (NBX_ERR_STATE at the next evaluation otherwise).  Same kernel with v_rsq_f32 in
 * place of v_rcp_f32 and one more multiply.  Forces, kick/drift, energy and the accuracy metric all follow the law. */
enum { NBX_FORCE_LAW_REFERENCE = 0, NBX_FORCE_LAW_NEWTON = 1 };
int nbx_ctx_set_law(nbx_ctx* ctx, int law);
/* PRECISION.  The reference's arithmetic is fp64 throughout (vector.h:9-12, methods.cpp:21-37); the device computes pair terms
 * in fp32 (stated tolerance: DESIGN.md section 4).  Two ways to go beyond plain fp32, both on the reference law -- the second is
 * what every context starts with (1e-5):
 *  - the variant "strict_f64_t4" (nbx_ctx_set_tuning): EVERY pair term, the skip-rule comparison and every sum in fp64 on
 *    the device's fp32-representable positions and masses -- agrees with brute_force_seq_n_body on the same inputs to
 *    ~1e-13 relative; about 2.5x the default kernel's time;
 *  - MIXED MODE, nbx_ctx_set_refine(ctx, rel_tolerance, sigma_factor): fp32 for every target, then the targets whose fp32
 *    sum cannot be trusted to rel_tolerance are re-evaluated by the strict kernel.  The criterion (force_kernel.hip,
 *    refine_select_kernel): the rounding error of a target's fp32 sum has standard deviation ~ c u sqrt(Q_i), u = 2^-24,
 *    Q_i = sum over the 64-source blocks of |block partial sum|^2 (accumulated by the default three-level kernel at no measurable
 *    cost; the two-level variant "fastpk_t8_w3_u4" sums over its 256-source tiles);
 *    target i is re-evaluated when  rel_tolerance |a_i| < sigma_factor u sqrt(Q_i)  -- a chance cancellation: the blocks'
 *    pulls add up to far less than they are -- or when it is a close-set target.  sigma_factor = 0 takes the library's
 *    calibrated default (nbx_refine_sigma_default).  rel_tolerance = 0 switches the mode off; a new context starts with the
 *    process default (nbx_set_default_refine: 1e-5 unless changed).  Ignored with a softening length, the
 *    Newtonian law, or a non-fast variant.  EVERY selected target is re-evaluated: the fp64 pass has room for the whole
 *    shard (its source slices shrink as the list grows, on the device) -- nbx_ctx_refine_stats reports the count. */
int nbx_ctx_set_refine(nbx_ctx* ctx, double rel_tolerance, double sigma_factor);
/* After a mixed-mode force evaluation: selected = targets the rule listed, refined = those re-evaluated in fp64
 * (the same number: there is no capacity to overflow).  Either pointer may be NULL.  Synchronises the stream. */
int nbx_ctx_refine_stats(nbx_ctx* ctx, unsigned* selected, unsigned* refined);
/* The per-target statistic the last force evaluation wrote beside the accelerations, double[count] (count as for nbx_ctx_get_forces):
 *   mixed mode:                  Q_i = sum over the source blocks of |block partial sum|^2 (what the selection rule thresholds);
 *   variant "strict_f64_t4_mag": S_i = sum_j |a_ij|, the sum of the pair terms' magnitudes (the yardstick of a cancelling
 *                                sum's error: backward error = |da_i| / S_i, condition number kappa_i = S_i / |a_i|).
 * NBX_ERR_STATE after any other evaluation.  Synchronises the stream. */
int nbx_ctx_get_aux(nbx_ctx* ctx, double* out);
/* The variant and slice count the next force evaluation will use (after upload).  A single-shard context that was given
 * neither a variant nor a slice count reports "sympk3l_t8_w3" -- the symmetric own-shard pass, every unordered pair evaluated
 * once -- where its shard has 8 to 255 super-blocks of 8,192 bodies, and then the pass's S + K slots as the slice count
 * (DESIGN.md section 3); nbx_default_variant() keeps naming the one-sided kernel that every other context runs.  A context
 * that was ASKED for "sympk3l_t8_w3" where the pass does not apply (a multi-shard context, fewer than two or more than 255
 * super-blocks) reports that name and runs the one-sided three-level kernel: the same pairs in the same arithmetic. */
int nbx_ctx_effective_tuning(nbx_ctx* ctx, int* variant, int* source_splits);
int nbx_num_variants(void);
const char* nbx_variant_name(int variant);
int nbx_default_variant(void);

/* Mean duration in ms of the force-kernel launches since the last call (hipEvent pairs recorded on
 * the context's stream around each launch), and how many launches that covers.  Synchronises. */
int nbx_ctx_kernel_time(nbx_ctx* ctx, float* mean_ms, int* launches);
/* Device time in ms (total, not mean) of the mixed mode's select / fp64 re-evaluation / fold kernels that followed the force-kernel
 * launches covered by the LAST nbx_ctx_kernel_time call (graph-replayed steps carry theirs inside the whole-step time). */
int nbx_ctx_refine_time(nbx_ctx* ctx, float* total_ms);

/* ---- MEASUREMENT entries (bench.py, tools/; nothing on the product path calls them) ----------------------------------
 * The symbol of the force kernel that an evaluation with `variant` (nbx_ctx_effective_tuning) launches for `dim`, in its plain
 * (mixed_mode = 0) or mixed-mode (1: also writes the spread sums) reference-law build, demangled as rocprofv3 prints it (e.g.
 * "void nbx::(anonymous namespace)::accel_fast3l_kernel<3, 4, 3, 4, 64, 1, 0, 1>(nbx::KArgs)"): what ties a live run to the
 * committed profiles/ of the same kernel.  Needs no device.  len >= 16 (NBX_ERR_INVALID otherwise; the name is truncated to fit). */
int nbx_variant_kernel_symbol(int variant, int dim, int mixed_mode, char* buf, size_t len);
/* In-kernel clock stamps: while on, every workgroup of the default (three-level) force kernel reads the shader clock
 * (s_memtime) and the constant 100 MHz clock (s_memrealtime) around its work -- two scalar loads and one 16-byte store per
 * workgroup of ~40 ms; no measurable cost (profiles/r5) -- and nbx_ctx_shader_clock reports, for the LAST stamped launch, the
 * median / smallest / largest of  d s_memtime / d s_memrealtime x 100 MHz  over its workgroups: the clock the chip actually
 * held under THIS kernel on THIS box, which is what a roofline fraction quoted at the 2.4 GHz peak cannot say.
 * NBX_ERR_STATE when the kernel that would run carries no stamps (non-default variants) or nothing stamped has run.
 * nbx_ctx_shader_clock synchronises the stream.  Any out pointer may be NULL. */
int nbx_ctx_enable_clock_stamps(nbx_ctx* ctx, int on);
int nbx_ctx_shader_clock(nbx_ctx* ctx, double* median_mhz, double* min_mhz, double* max_mhz, int* workgroups);
/* The same box's ceiling: a pure v_pk_fma_f32 stream (16 independent chains per lane, 24 workgroups of 256 lanes per CU, as many resident as fit)
 * for about target_ms (1..2000) on `device`; *tflops = what it achieved (4 flop per lane-instruction), *shader_mhz = the
 * clock it held.  The guide's 157.3 TFLOP/s assumes 2.4 GHz and one packed FMA per cycle per lane pair. */
int nbx_measure_valu_ceiling(int device, double target_ms, double* tflops, double* shader_mhz);

/* ---- single-process multi-GPU node ---------------------------------------------------------------
 * The reference is single-process, single-device; this is new.  One context per rank
 * (n_shards = n_ranks, shard = rank) on devices[rank] (NULL: 0..n_ranks-1; a device may appear more than
 * once -- "virtual ranks", used to rehearse the sharded path on one GPU), driven by the calling thread.
 * Per step every rank's freshly drifted fp32 position chunk is all-gathered on a second HIP stream while
 * the rank's compute stream evaluates the forces from its own chunk; the pass over the other ranks'
 * chunks waits on the exchange's event.  exchange: RCCL = ncclAllGather over one communicator per node
 * (librccl is dlopen'ed on demand; needs distinct devices), PEER_COPY = every rank pushes its chunk into
 * each peer's buffer with hipMemcpyPeerAsync, AUTO = RCCL when n_ranks > 1 distinct devices, else PEER_COPY.
 * The one-process-per-GPU twin of this layer is nbody-simulation-parallel_amd/dist.py. */
typedef struct nbx_node nbx_node;
enum { NBX_EXCHANGE_AUTO = 0, NBX_EXCHANGE_PEER_COPY = 1, NBX_EXCHANGE_RCCL = 2 };
int nbx_node_create(nbx_node** out, int n_ranks, const int* devices, int dim, size_t n_total, int exchange);
int nbx_node_destroy(nbx_node* node);
int nbx_node_exchange_mode(const nbx_node* node, int* mode);
/* `bodies` is the whole Body<D> array; each rank copies only its own shard of it to its device, the other chunks of its
 * source copy arrive device to device (masses once, positions through the step's exchange).  With the RCCL exchange and
 * more than one rank the first upload over a communicator set also runs nbx_node_verify_exchange and fails (NBX_ERR_HIP,
 * detail text) if the all-gather did not deliver every chunk. */
int nbx_node_upload_bodies(nbx_node* node, const void* bodies, size_t body_stride_bytes);
/* Self-check of the position exchange: every rank's copies of the chunks it does not own are overwritten with
 * NaN, one exchange runs (RCCL all-gather or peer copies, as configured), and each copy is compared bit for bit
 * with the owner's chunk on the host.  *mismatches = number of differing fp32 values over all ranks (0 = the
 * exchange delivered every chunk everywhere).  Synchronises; leaves the buffers whole when it passes. */
int nbx_node_verify_exchange(nbx_node* node, size_t* mismatches);
int nbx_node_set_tuning(nbx_node* node, int source_splits, int variant);
int nbx_node_set_softening(nbx_node* node, double epsilon);   /* nbx_ctx_set_softening on every rank */
int nbx_node_set_law(nbx_node* node, int law);                /* nbx_ctx_set_law on every rank */
int nbx_node_set_refine(nbx_node* node, double rel_tolerance, double sigma_factor);   /* nbx_ctx_set_refine on every rank */
/* nbx_ctx_refine_stats summed over the ranks (after nbx_node_compute_forces / a step); NBX_ERR_STATE when no rank ran the mixed mode. */
int nbx_node_refine_stats(nbx_node* node, unsigned* selected, unsigned* refined);
/* Forces on all n_total bodies (Vector<dim>[n_total]); same contract as nbx_brute_force_forces. */
int nbx_node_compute_forces(nbx_node* node, double G, double* forces_out);
/* nsteps x { exchange || local forces; remote forces; kick+drift } on every rank.  Asynchronous. */
int nbx_node_step(nbx_node* node, double G, double dt, int nsteps);
int nbx_node_step_kdk(nbx_node* node, double G, double dt, int nsteps);   /* kick-drift-kick form, see nbx_ctx_step_kdk */
int nbx_node_synchronize(nbx_node* node);
int nbx_node_download_bodies(nbx_node* node, void* bodies, size_t body_stride_bytes);
int nbx_node_energy(nbx_node* node, double G, double* kinetic, double* potential);
int nbx_node_kernel_time(nbx_node* node, float* mean_ms, int* launches);
/* Self-description of a sharded evaluation (what a first run on a multi-GPU node prints): with timing enabled every evaluation
 * records events around each rank's LOCAL and REMOTE pass (compute stream) and around its part of the exchange (comm stream);
 * nbx_node_pass_times reports the LAST evaluation's figures for `rank` -- device, targets, the three durations in ms, and whether
 * the exchange had finished before the LOCAL pass did (exchange_hidden).  Any out pointer may be NULL.  Synchronises. */
int nbx_node_enable_timing(nbx_node* node, int on);
int nbx_node_pass_times(nbx_node* node, int rank, int* device, size_t* targets, float* local_ms, float* remote_ms,
                        float* exchange_ms, int* exchange_hidden);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_H */
