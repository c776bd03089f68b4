"""GPU: the adaptive octree built on the device (nbx_leaf_plan_create_octree_adaptive, csrc/octree_device.hip) against its
specification, the host builder leaves.adaptive_octree_cells: the eight arrays word for word on every named input, size edge and at
N = 2^20; forces bit for bit against a plan made from the host arrays; near + far against the oracle on the augmented system (method
and tolerance of tests/test_gpu_far_field.py); brute force at theta = 0; step loops; reuse; refusals; the C++ layer and the harness;
and the accuracy of the tree against all-pairs sums next to the fixed-depth tree's.

theta = 0 puts every leaf on every near list, so those runs take the first 2,000 bodies of an input (as the CPU twin does)."""
import math
import os
import subprocess

import numpy as np
import pytest

import octree_inputs
from oracle_lib import assert_force_parity
from test_gpu_far_field import assert_far_parity, augmented, moments, planner, rounding_allowance
from test_gpu_octree_device import NBX_ERR_INVALID, NBX_ERR_STATE, assert_same_structure

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nbody-simulation-parallel_amd")
CAPACITIES = (1, 16, 64)
THETA_ZERO_BODIES = 2000


def device_structure(nbx, b, dim, max_depth, cap, theta):
    n = b.shape[0]
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta) as plan:
            return plan.structure(), plan.structure_sizes()


def check_word_for_word(nbx, b, dim, max_depth, cap, theta, what):
    want = nbx.leaves.adaptive_octree_cells(b, dim, max_depth, cap, theta)
    got, sizes = device_structure(nbx, b, dim, max_depth, cap, theta)
    assert_same_structure(got, want, what)
    assert sizes == (want[0].size - 1, want[3].size, want[4].size, want[7].size), what
    return want


def plummer(nbx, oracle, n, dim=3, seed=1):
    return oracle.round_inputs_to_f32(nbx.generate.plummer_bodies(n, dim, seed))


GEOMETRY = [(name, dim, n, seed, depths, md) for name, dim, n, seed, depths in octree_inputs.GEOMETRY_CASES for md in dict.fromkeys(tuple(depths) + (10,))]


@pytest.mark.parametrize("name,dim,n,seed,depths,max_depth", GEOMETRY, ids=[f"{c[0]}-{c[1]}d-maxdepth{c[5]}" for c in GEOMETRY])
def test_structure_of_every_named_input(nbx, oracle, name, dim, n, seed, depths, max_depth):
    full = octree_inputs.GENERATORS[name](oracle, dim, n, seed, depths[0])
    for cap in CAPACITIES:
        check_word_for_word(nbx, full, dim, max_depth, cap, 0.5, f"{name} {dim}D max_depth {max_depth} capacity {cap} theta 0.5")
    # the other two opening angles of the CPU twin at the middle capacity
    check_word_for_word(nbx, full, dim, max_depth, 16, 0.9, f"{name} {dim}D max_depth {max_depth} capacity 16 theta 0.9")
    check_word_for_word(nbx, full[:THETA_ZERO_BODIES], dim, max_depth, 16, 0.0, f"{name} {dim}D max_depth {max_depth} capacity 16 theta 0")


@pytest.mark.parametrize("n", octree_inputs.SIZES)
def test_structure_at_every_size_edge(nbx, oracle, n):
    b = octree_inputs.size_case(oracle, n)
    for max_depth in octree_inputs.SIZE_DEPTHS + (10,):
        check_word_for_word(nbx, b, 3, max_depth, 16, 0.5, f"n {n} max_depth {max_depth} capacity 16")


@pytest.mark.parametrize("kind", ("plummer", "uniform"))
def test_structure_at_size(nbx, oracle, kind):
    n = 1 << 20
    b = plummer(nbx, oracle, n) if kind == "plummer" else oracle.round_inputs_to_f32(oracle.generate(77, n, 3))
    want = check_word_for_word(nbx, b, 3, 10, 32, 0.5, f"{kind} N = 2^20 capacity 32")
    sizes = np.diff(want[0].astype(np.int64))
    print(f"\n{kind} N = 2^20 capacity 32: {sizes.size} leaves, largest {int(sizes.max())}, near entries {want[3].size}, cells {want[4].size}, far entries {want[7].size}")
    assert int(sizes.max()) == 32


@pytest.mark.parametrize("dim,max_depth,theta", ((3, 4, 0.5), (3, 10, 0.7), (2, 6, 0.5), (3, 0, 0.5), (3, 3, 0.0)))
def test_capacity_zero_is_the_fixed_depth_plan(nbx, oracle, dim, max_depth, theta):
    n = 20000 if theta > 0.0 else 4096
    b = oracle.round_inputs_to_f32(oracle.generate(320 + max_depth, n, dim))
    want = nbx.leaves.octree_cells(b, dim, max_depth, theta)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree(c, max_depth, theta) as fixed, nbx.LeafPlan.from_octree_adaptive(c, max_depth, 0, theta) as plan:
            assert_same_structure(plan.structure(), fixed.structure(), "capacity 0 against from_octree")
            assert_same_structure(plan.structure(), want, "capacity 0 against octree_cells")
            assert plan.structure_sizes() == fixed.structure_sizes()
            assert np.array_equal(plan.forces_ctx(c, nbx.LAW_TREE_LEAF, oracle.G), fixed.forces_ctx(c, nbx.LAW_TREE_LEAF, oracle.G))
            plan.rebuild(c)
            assert_same_structure(plan.structure(), want, "capacity 0 rebuilt")


def host_plan(nbx, n, dim, s):
    with planner("device"):
        ref = nbx.LeafPlan(n, dim, *s[:4])
        ref.set_cells(*s[4:])
    return ref


BIT_CASES = (("uniform", 20000, 3, 10, 16, 0.5), ("uniform", 20000, 2, 10, 16, 0.5), ("clustered", 60000, 3, 7, 16, 0.5), ("clustered", 60000, 2, 10, 64, 0.7),
             ("plummer", 131072, 3, 10, 32, 0.5), ("plummer", 20000, 2, 10, 1, 0.5), ("uniform", 5000, 3, 6, 5000, 0.5))


@pytest.mark.parametrize("law_name", ("LAW_TREE_LEAF", "LAW_FMM_P2P"))
@pytest.mark.parametrize("kind,n,dim,max_depth,cap,theta", BIT_CASES)
def test_same_bits_as_the_host_array_path(nbx, oracle, kind, n, dim, max_depth, cap, theta, law_name):
    if kind == "plummer":
        b = plummer(nbx, oracle, n, dim)
    else:
        b = octree_inputs.GENERATORS[kind](oracle, dim, n, 330 + dim)
    law = getattr(nbx, law_name)
    host = nbx.leaves.adaptive_octree_cells(b, dim, max_depth, cap, theta)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with host_plan(nbx, n, dim, host) as ref, nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta) as plan:
            assert_same_structure(plan.structure(), host, f"{kind} {dim}D")
            assert plan.info() == ref.info()
            assert plan.cell_info()[:2] == ref.cell_info()[:2]
            want = ref.forces_ctx(c, law, oracle.G)
            got = plan.forces_ctx(c, law, oracle.G)
            assert np.array_equal(got, want), f"{int((got != want).any(axis=1).sum())} bodies differ"
            assert np.array_equal(plan.get_forces(), want)
            if host[4].size:
                for g, w in zip(plan.cells(), ref.cells()):
                    assert np.array_equal(g, w)
            assert np.isfinite(got).all() and np.any(got != 0.0)


@pytest.mark.parametrize("law", (0, 1, 2))
@pytest.mark.parametrize("kind,dim,cap,theta", (("uniform", 3, 16, 0.5), ("plummer", 3, 16, 0.7), ("uniform", 2, 4, 0.5)))
def test_near_plus_far_against_the_augmented_oracle(nbx, oracle, kind, dim, cap, theta, law):
    """tests/test_gpu_far_field.py's check on the adaptive structure, the plan built on the device: the oracle sums the bodies and one
    pseudo-body per cell; the tolerance is that file's (oracle_lib's constants plus the fp32 rounding of the pseudo-bodies)."""
    n, max_depth = 20000, 10
    b = plummer(nbx, oracle, n, dim, 3) if kind == "plummer" else oracle.round_inputs_to_f32(oracle.generate(50 + dim, n, dim))
    s = nbx.leaves.adaptive_octree_cells(b, dim, max_depth, cap, theta)
    leaves, cells, far = s[:4], s[4:6], s[6:8]
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta) as plan:
            assert_same_structure(plan.structure(), s, kind)
            f = plan.forces_ctx(c, law, oracle.G)
    mass, com = moments(b, dim, leaves, cells)
    b2, leaves2 = augmented(b, dim, leaves, cells, far, mass, com)
    ref = oracle.leaf_pair_forces(b2, leaves2, law)[:n]
    S = oracle.leaf_pair_magnitude_sums(b2, leaves2, law)[:n]
    E = rounding_allowance(b, dim, leaves, far, mass, com, oracle.G)
    assert_far_parity(f, ref, S, E, f"adaptive {kind} D={dim} capacity {cap} theta {theta} law {law}")


def test_theta_zero_is_brute_force(nbx, oracle):
    n, dim = 4096, 3
    b = oracle.round_inputs_to_f32(oracle.generate(303, n, dim))
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree_adaptive(c, 10, 16, 0.0) as plan:
            nl, near, nc, far = plan.structure_sizes()
            assert near == nl * nl and far == 0 and nl > n // 16
            f = plan.forces_ctx(c, 0, oracle.G)
    assert_force_parity(f, oracle.brute_force_seq(b), oracle.force_magnitude_sums(b), "adaptive octree plan at theta = 0 vs sequential reference")


def host_loop(nbx, b0, dim, max_depth, cap, theta, law, G, dt, steps, rebuild_every):
    """Per step: bodies down, adaptive_octree_cells on them (when the step rebuilds), a fresh LeafPlan + set_cells, forces, kick_drift."""
    n = b0.shape[0]
    cur = b0.copy()
    structures = []
    with nbx.Context(n, dim) as c:
        c.upload(b0)
        plan = None
        for k in range(steps):
            if plan is None or (rebuild_every > 0 and k % rebuild_every == 0):
                if plan is not None:
                    plan.close()
                c.download(cur)
                s = nbx.leaves.adaptive_octree_cells(cur, dim, max_depth, cap, theta)
                structures.append(s)
                plan = host_plan(nbx, n, dim, s)
            plan.forces_ctx(c, law, G, fetch=False)
            plan.kick_drift(c, dt)
        c.download(cur)
        plan.close()
    return cur, structures


@pytest.mark.parametrize("law_name", ("LAW_TREE_LEAF", "LAW_FMM_P2P"))
@pytest.mark.parametrize("dim", (2, 3))
def test_step_loops(nbx, oracle, dim, law_name):
    """7 steps rebuilding every 0 (never), 1 and 3 (at steps 0, 3 and 6): nbx_leaf_plan_step_octree against the explicit
    rebuild / forces / kick-drift calls on the same plan, and against the host-array loop fed the downloaded positions."""
    n, max_depth, cap, theta, dt, steps = 20000, 10, 16, 0.5, 1.5, 7
    law, G = getattr(nbx, law_name), oracle.G * 1e26
    b0 = oracle.round_inputs_to_f32(oracle.generate(340 + dim, n, dim))
    b0[:, dim:2 * dim] *= 1000.0
    for every in (0, 1, 3):
        want, structures = host_loop(nbx, b0, dim, max_depth, cap, theta, law, G, dt, steps, every)
        assert len(structures) == {0: 1, 1: 7, 3: 3}[every]
        got, explicit = b0.copy(), b0.copy()
        with nbx.Context(n, dim) as c:
            c.upload(b0)
            with nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta) as plan:
                plan.step_octree(c, law, G, dt, steps, every)
                c.download(got)
                last = plan.structure()
        with nbx.Context(n, dim) as c:
            c.upload(b0)
            with nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta) as plan:
                for k in range(steps):
                    if every > 0 and k % every == 0:
                        plan.rebuild(c)
                    plan.forces_ctx(c, law, G, fetch=False)
                    plan.kick_drift(c, dt)
                c.download(explicit)
        assert np.array_equal(got, explicit), f"rebuilding every {every}: step_octree against the explicit calls"
        assert np.array_equal(got, want), f"rebuilding every {every}: {int((got != want).any(axis=1).sum())} bodies differ from the host-array loop"
        assert_same_structure(last, structures[-1], f"last structure, rebuilding every {every}")
        assert not np.array_equal(got[:, :dim], b0[:, :dim])
        if every > 0:
            assert not np.array_equal(structures[-1][1], structures[0][1]), "the bodies did not change leaves: the test shows nothing"


def test_determinism_and_reuse(nbx, oracle):
    n, dim, max_depth = 20000, 3, 10
    b = plummer(nbx, oracle, n, dim, 5)
    wide, narrow = nbx.leaves.adaptive_octree_cells(b, dim, max_depth, 16, 0.9), nbx.leaves.adaptive_octree_cells(b, dim, max_depth, 16, 0.3)
    assert narrow[3].size > 2 * wide[3].size, "the two list volumes are too close to test reuse"
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 16, 0.9) as pa, nbx.LeafPlan.from_octree_adaptive(c, max_depth, 16, 0.9) as pb:
            first = pa.structure()
            assert_same_structure(pb.structure(), first, "a second build")
            assert_same_structure(first, wide, "theta 0.9")
            want = pa.forces_ctx(c, 1, oracle.G)
            pa.rebuild(c)
            assert_same_structure(pa.structure(), wide, "theta 0.9 rebuilt")
            assert np.array_equal(pa.forces_ctx(c, 1, oracle.G), want)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 16, 0.3) as pc:
            assert_same_structure(pc.structure(), narrow, "theta 0.3 after theta 0.9")
            pc.rebuild(c)
            assert_same_structure(pc.structure(), narrow, "theta 0.3 rebuilt")
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 16, 0.9) as pd:
            assert_same_structure(pd.structure(), wide, "theta 0.9 after theta 0.3")
            assert np.array_equal(pd.forces_ctx(c, 1, oracle.G), want)
        # the same plan across a change of every array's size: half of the bodies contract to a hundredth, then come back
        small = b.copy()
        small[: n // 2, :dim] *= 0.01
        small = oracle.round_inputs_to_f32(small)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 64, 0.5) as pe:
            c.upload(small)
            pe.rebuild(c)
            assert_same_structure(pe.structure(), nbx.leaves.adaptive_octree_cells(small, dim, max_depth, 64, 0.5), "rebuilt on contracted bodies")
            c.upload(b)
            pe.rebuild(c)
            assert_same_structure(pe.structure(), nbx.leaves.adaptive_octree_cells(b, dim, max_depth, 64, 0.5), "rebuilt on the first bodies: the plan kept its capacity")


def test_refusals(nbx, oracle):
    n, dim = 5000, 3
    b = oracle.round_inputs_to_f32(oracle.generate(306, n, dim))
    want = nbx.leaves.adaptive_octree_cells(b, dim, 10, 16, 0.5)

    def refused(status, make):
        with pytest.raises(nbx.NbxError) as e:
            make()
        assert e.value.status == status, str(e.value)

    def valid(c):
        with nbx.LeafPlan.from_octree_adaptive(c, 10, 16, 0.5) as plan:
            assert_same_structure(plan.structure(), want, "a valid build after a refusal")

    with nbx.Context(n, dim) as c:
        refused(NBX_ERR_STATE, lambda: nbx.LeafPlan.from_octree_adaptive(c, 10, 16, 0.5))          # nothing uploaded yet
        c.upload(b)
        valid(c)
        for max_depth, cap, theta in ((11, 16, 0.5), (-1, 16, 0.5), (10, -1, 0.5), (10, 16, -0.1), (10, 16, float("nan")), (10, 16, float("inf"))):
            refused(NBX_ERR_INVALID, lambda: nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta))
            valid(c)
        with nbx.Context(n, dim, 0, 2, 0) as two:
            refused(NBX_ERR_INVALID, lambda: nbx.LeafPlan.from_octree_adaptive(two, 10, 16, 0.5))
        valid(c)
        bad = b.copy()
        bad[n // 2, 1] = float("nan")
        try:
            c.upload(bad)
        except nbx.NbxError:
            pytest.fail("the context refused the upload: the builder's own check was not reached")
        refused(NBX_ERR_INVALID, lambda: nbx.LeafPlan.from_octree_adaptive(c, 10, 16, 0.5))
        c.upload(b)
        valid(c)
        with nbx.LeafPlan.from_octree_adaptive(c, 10, 16, 0.5) as plan:
            c.upload(bad)
            refused(NBX_ERR_INVALID, lambda: plan.rebuild(c))
            refused(NBX_ERR_STATE, lambda: plan.forces_ctx(c, 1, oracle.G))
            refused(NBX_ERR_STATE, lambda: plan.structure())
            c.upload(b)
            plan.rebuild(c)
            assert_same_structure(plan.structure(), want, "rebuilt after a refused rebuild")


def test_too_many_near_entries_are_refused(nbx, oracle):
    """theta = 0 puts every leaf on every near list: n_leaves^2 entries.  70,000 bodies at capacity 1 and max_depth 10 give (counted on
    the host first, from the distinct finest cells) more than 65,536 leaves, so more than 0xfffffff0 entries: NBX_ERR_INVALID
    before any list is written, from the create call and from a rebuild, after which the plan is in NBX_ERR_STATE."""
    n, dim, max_depth = 70000, 3, 10
    b = oracle.round_inputs_to_f32(oracle.generate(350, n, dim))
    nl = nbx.leaves.adaptive_octree_cells(b, dim, max_depth, 1, 4.0)[0].size - 1      # the leaves do not depend on theta; a wide one keeps the host's lists short
    assert nl * nl > 0xfffffff0, f"{nl} leaves: the input does not cross the limit"
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with pytest.raises(nbx.NbxError) as e:
            nbx.LeafPlan.from_octree_adaptive(c, max_depth, 1, 0.0)
        assert e.value.status == NBX_ERR_INVALID and "too long" in str(e.value), str(e.value)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 64, 0.5) as ok:
            want = ok.structure()
        # a plan whose parameters cross the limit only once the bodies have spread: built on a few cells, rebuilt on all of them
        packed = b.copy()
        packed[:, :dim] = b[:8, :dim][np.arange(n) % 8]
        c.upload(packed)
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 1, 0.0) as plan:
            assert plan.structure_sizes()[0] <= 8
            c.upload(b)
            with pytest.raises(nbx.NbxError) as e:
                plan.rebuild(c)
            assert e.value.status == NBX_ERR_INVALID
            with pytest.raises(nbx.NbxError) as e:
                plan.forces_ctx(c, 1, oracle.G)
            assert e.value.status == NBX_ERR_STATE
        with nbx.LeafPlan.from_octree_adaptive(c, max_depth, 64, 0.5) as again:
            assert_same_structure(again.structure(), want, "a valid build after the refusals")


def test_cpp_layer_and_harness(nbx, oracle, tmp_path):
    """barnes_hut_hip_adaptive_n_body<D> and _steps<D> (tests/adaptive_octree_cpp_check.cpp, built here) give the forces and the bodies
    of the Python plan bit for bit; nbody_sim -m t --leaf-cap 32 on a small Plummer input writes its two rows, reports the leaves
    and passes its accuracy check; without --leaf-cap the rows are not written."""
    n, theta, cap, max_depth = 20000, 0.5, 32, 10
    exe = str(tmp_path / "adaptive_octree_cpp_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"),
                    os.path.join(ROOT, "tests", "adaptive_octree_cpp_check.cpp"), os.path.join(PKG, "host", "leaf_pairs_hip.cpp"), "-o", exe,
                    "-L" + PKG, "-lnbody_hip", "-Wl,-rpath," + PKG], check=True, capture_output=True, text=True)
    for d in (2, 3):
        bd = plummer(nbx, oracle, n, d, 11)
        bd[:, d:2 * d] *= 1000.0
        path, res = str(tmp_path / f"bodies{d}.f64"), str(tmp_path / f"out{d}.f64")
        np.ascontiguousarray(bd).tofile(path)
        stepped = bd.copy()
        with nbx.Context(n, d) as c:
            c.upload(bd)
            with nbx.LeafPlan.from_octree_adaptive(c, max_depth, cap, theta) as plan:
                fd = plan.forces_ctx(c, nbx.LAW_TREE_LEAF, oracle.G)
                plan.step_octree(c, nbx.LAW_TREE_LEAF, oracle.G, 1.5, 5, 2)
                c.download(stepped)
        assert not np.array_equal(stepped[:, :d], bd[:, :d])
        p = subprocess.run([exe, str(d), path, str(n), str(max_depth), str(cap), repr(theta), res], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert np.array_equal(np.fromfile(res).reshape(n, d), fd), f"barnes_hut_hip_adaptive_n_body<{d}>"
        p = subprocess.run([exe, str(d), path, str(n), str(max_depth), str(cap), repr(theta), res + ".steps", "steps", "1.5", "5", "2"],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert np.array_equal(np.fromfile(res + ".steps").reshape(n, 2 * d + 1), stepped), f"barnes_hut_hip_adaptive_steps<{d}>"
    sim = os.path.join(ROOT, "nbody_sim")
    assert os.path.exists(sim)

    def rows_of(folder, *extra):
        os.makedirs(folder)
        p = subprocess.run([sim, "-N", "20000", "--init", "plummer", "-m", "t", "-a", "1", "--theta", "0.3", "--steps", "3", *extra],
                           cwd=folder, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        found = [os.path.join(d_, f_) for d_, _, files in os.walk(folder) for f_ in files if f_.endswith(".csv")]
        return {line.split(",")[0]: line.strip().split(",") for path in found for line in open(path) if line.startswith("BarnesHut_HIP")}, p.stdout

    rows, text = rows_of(str(tmp_path / "adaptive"), "--leaf-cap", "32")
    assert set(rows) == {"BarnesHut_HIP_adaptive", "BarnesHut_HIP_adaptive_steps"}, text
    accuracy = float(rows["BarnesHut_HIP_adaptive"][-1])
    print(f"\nBarnesHut_HIP_adaptive row: {rows['BarnesHut_HIP_adaptive']}; accuracy against the brute-force forces {accuracy} %")
    assert math.isfinite(accuracy) and 0.0 <= accuracy <= 100.0
    report = [line for line in text.splitlines() if line.startswith("Leaves: ")]
    assert len(report) == 1, text
    leaves, largest = int(report[0].split()[1].rstrip(",")), int(report[0].split()[4])
    assert largest <= 32 and leaves >= 20000 // 32, report
    assert "Error executing" not in text
    rows, text = rows_of(str(tmp_path / "fixed"))
    assert set(rows) == {"BarnesHut_HIP"}, text


def relative_errors(f, ref):
    return np.sqrt(((f - ref) ** 2).sum(axis=1)) / np.sqrt((ref ** 2).sum(axis=1))


def tree_errors(nbx, oracle, b, rows, make):
    """Median and 99th percentile of |F_tree - F_all| / |F_all| over `rows`: TREE_LEAF sums (attractive) against the oracle's all-pairs
    sums (repulsive: the sign is turned)."""
    n = b.shape[0]
    with nbx.Context(n, 3) as c:
        c.upload(b)
        with make(c) as plan:
            f = plan.forces_ctx(c, nbx.LAW_TREE_LEAF, oracle.G)
            nl = plan.structure_sizes()[0]
    err = relative_errors(f[rows], -oracle.force_rows_omp_2(b, rows))
    return float(np.median(err)), float(np.percentile(err, 99.0)), nl


def test_accuracy_against_all_pairs(nbx, oracle):
    """Uniform, N = 131,072, theta 0.5: the adaptive tree at capacity 16 is the fixed tree of depth 5 but for 0.1 % of its leaves, so its
    median and 99th-percentile relative force errors (4,096 sampled bodies, against all-pairs sums) must stay within 1.5 x of the
    fixed tree's on the same bodies.  Plummer: the same figures are printed and not asserted (the fixed tree sums half of all pairs
    directly there, which makes it no yardstick)."""
    n, theta = 131072, 0.5
    rows = np.sort(np.random.default_rng(9).choice(n, 4096, replace=False))
    depth = 5                                                       # barnes_hut_hip_depth(131072, 3)
    b = oracle.round_inputs_to_f32(oracle.generate(1, n, 3))
    fixed = tree_errors(nbx, oracle, b, rows, lambda c: nbx.LeafPlan.from_octree(c, depth, theta))
    adaptive = tree_errors(nbx, oracle, b, rows, lambda c: nbx.LeafPlan.from_octree_adaptive(c, 10, 16, theta))
    print(f"\nuniform N = {n} theta {theta}: fixed depth {depth}: median {fixed[0]:.3e} p99 {fixed[1]:.3e} ({fixed[2]} leaves); "
          f"adaptive capacity 16: median {adaptive[0]:.3e} p99 {adaptive[1]:.3e} ({adaptive[2]} leaves)")
    p = plummer(nbx, oracle, n)
    for cap in (16, 32, 64):
        e = tree_errors(nbx, oracle, p, rows, lambda c: nbx.LeafPlan.from_octree_adaptive(c, 10, cap, theta))
        print(f"Plummer N = {n} theta {theta}: adaptive capacity {cap}: median {e[0]:.3e} p99 {e[1]:.3e} ({e[2]} leaves)")
    e = tree_errors(nbx, oracle, p, rows, lambda c: nbx.LeafPlan.from_octree(c, depth, theta))
    print(f"Plummer N = {n} theta {theta}: fixed depth {depth}: median {e[0]:.3e} p99 {e[1]:.3e} ({e[2]} leaves)")
    assert adaptive[0] <= 1.5 * fixed[0] and adaptive[1] <= 1.5 * fixed[1]
