"""GPU: the device octree builder (csrc/octree_device.hip) word for word against leaves.octree_cells where
tests/test_gpu_octree_device.py does not go: every count of radix passes of the key sort (0 .. 4, and the key widths next to
each change), body counts on both sides of every tile edge of the builder's kernels, the named inputs of tests/octree_inputs.py
(bodies on grid planes and box faces, degenerate boxes, signs, scales, duplicates) at an even and an odd pass count, opening
angles whose acceptance test ties exactly on the integer lattice, N = 2^20 at depth 6, and the refusals of near and of far lists beyond
2^32 entries.  The tolerance is that module's: exact equality of the eight arrays and of structure_sizes().  Every self-check of an
input (boundary share, tie count, leaf-count residues, the near-entry lower bound) is computed on the host and asserted BEFORE
the device is asked; tests/test_octree_build_cpu.py runs the same inputs through the g++ build of the shared header."""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import octree_inputs
from octree_inputs import GENERATORS, passes
from test_gpu_octree_device import NAMES, NBX_ERR_INVALID, assert_same_structure, check_word_for_word

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (dim, depth): key widths 0 | 2 8 | 10 16 18 20 | 0 | 3 6 | 9 15 | 18 21 24 | 27 30 bits
PASS_CASES = tuple((2, d) for d in (0, 1, 4, 5, 8, 9, 10)) + tuple((3, d) for d in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10))
assert {passes(dim, depth) for dim, depth in PASS_CASES} == {0, 1, 2, 3, 4}
assert {dim * depth for dim, depth in PASS_CASES} >= {8, 9, 10, 16, 18, 24, 27}      # both sides of 8 | 9, 16 | 17 and 24 | 25


@pytest.mark.parametrize("dim,depth", PASS_CASES)
def test_every_pass_count_word_for_word(nbx, oracle, dim, depth):
    b = octree_inputs.uniform(oracle, dim, 20000, 330 + 16 * dim + depth)
    want = check_word_for_word(nbx, b, dim, depth, 0.5, f"dim {dim} depth {depth}: {passes(dim, depth)} radix passes")
    print(f"\ndim {dim} depth {depth}: {dim * depth} key bits, {passes(dim, depth)} passes, {want[0].size - 1} leaves, {want[3].size} near, {want[7].size} far")


@pytest.mark.parametrize("depth", octree_inputs.SIZE_DEPTHS)
@pytest.mark.parametrize("n", octree_inputs.SIZES)
def test_sizes_at_the_tile_edges_word_for_word(nbx, oracle, n, depth):
    """3D, depth 3 (2 passes) and depth 6 (3 passes), n on both sides of 64, 256, 2048, 4096 and 65,536; the leaf counts the
    cases give are checked for their residues mod 64 in test_octree_build_cpu.py::test_size_cases_put_leaf_counts_on_the_wave_edges."""
    b = octree_inputs.size_case(oracle, n)
    want = check_word_for_word(nbx, b, 3, depth, 0.5, f"n = {n}, depth {depth}")
    print(f"\nn {n} depth {depth}: n_leaves {want[0].size - 1} (mod 64: {(want[0].size - 1) % 64}, mod 256: {(want[0].size - 1) % 256})")


GEOMETRY = [(name, dim, n, seed, depth) for name, dim, n, seed, depths in octree_inputs.GEOMETRY_CASES for depth in depths]


@pytest.mark.parametrize("name,dim,n,seed,depth", GEOMETRY, ids=[f"{c[0]}-{c[1]}d-depth{c[4]}" for c in GEOMETRY])
def test_named_inputs_word_for_word(nbx, oracle, name, dim, n, seed, depth):
    b = GENERATORS[name](oracle, dim, n, seed, depth)
    if name in ("planes", "lattice"):
        share = octree_inputs.share_on_grid_planes(b[:, :dim], depth)
        print(f"\n{name} dim {dim} depth {depth}: {share:.3f} of the bodies on a grid plane of the root box")
        assert share >= 1.0 / 3.0, "the input misses the planes it is made for"
    want = check_word_for_word(nbx, b, dim, depth, 0.5, f"{name}, dim {dim}, depth {depth} ({passes(dim, depth)} passes)")
    if name in ("one_point", "denormal"):
        assert want[0].size == 2
    if name == "clustered" and depth == 7:
        assert int(np.diff(want[0].astype(np.int64)).max()) > 256, "no leaf of more than 256 bodies"


THETAS = (1.0, 0.8, 0.25, 2.0, 100.0, 1e300, 1e-3)


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("dim,depth", ((3, 4), (2, 5)))
@pytest.mark.parametrize("name", ("lattice", "uniform"))
def test_opening_angles_that_tie_word_for_word(nbx, oracle, name, dim, depth, theta):
    """theta = 1 ties at gap = 2^s, 0.8 at gaps (3, 4, 0) 2^(s-2) and (5, 0, 0) 2^(s-2) [0.8 * 5 rounds to 4.0 exactly], 0.25 at
    gap = 2^(s+2); a tie is NOT accepted (strict <).  100 and 1e300 accept every node with a positive gap at level 1; 1e-3
    accepts nothing (the largest gap, 2^depth sqrt(3), times 1e-3 stays below 1)."""
    b = GENERATORS[name](oracle, dim, 20000, 440 + dim, depth)
    if name == "lattice" and theta in (1.0, 0.8, 0.25):
        ties = octree_inputs.count_exact_ties(nbx.leaves, b, dim, depth, theta)
        print(f"\n{name} dim {dim} depth {depth} theta {theta}: {ties} tested (leaf, node) pairs tie exactly")
        assert ties > 0, "no exact tie of the acceptance test: the case shows nothing"
    want = check_word_for_word(nbx, b, dim, depth, theta, f"{name}, dim {dim}, depth {depth}, theta {theta}")
    nl = want[0].size - 1
    if theta == 1e-3:
        assert want[7].size == 0 and want[3].size == nl * nl
    if theta == 1e300:
        # the device equals the host at 100 (its own case) and at 1e300 (above); the two host structures are the same one
        assert_same_structure(want, nbx.leaves.octree_cells(b, dim, depth, 100.0), "theta 1e300 against theta 100")


def structure_array(nbx, plan, k):
    """One of the eight arrays of plan.structure(), copied alone (nbx_leaf_plan_get_structure takes NULL for the others)."""
    nl, near, nc, far = plan.structure_sizes()
    out = np.zeros((nl + 1, plan.n, nl + 1, near, nc, nc, nl + 1, far)[k], dtype=np.uint32)
    args = [None] * 8
    args[k] = out.ctypes.data if out.size else None
    plan._ck(plan.lib.nbx_leaf_plan_get_structure(plan.h, *args), "nbx_leaf_plan_get_structure")
    return out


def test_structure_at_size_depth_6(nbx, oracle):
    """N = 2^20, seed 77, 3D, depth 6 (18 key bits: 3 passes), theta 0.5: the configuration of profiles/r7/octree_device.txt.
    far_cells is 2 GB a copy: one array at a time, each freed after its comparison."""
    n, dim, depth, theta = 1 << 20, 3, 6, 0.5
    b = oracle.round_inputs_to_f32(oracle.generate(77, n, dim))
    t0 = time.perf_counter()
    want = list(nbx.leaves.octree_cells(b, dim, depth, theta))
    print(f"\nhost builder {time.perf_counter() - t0:.1f} s: {want[0].size - 1} leaves, {want[3].size} near, {want[4].size} cells, {want[7].size} far")
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree(c, depth, theta) as plan:
            assert plan.structure_sizes() == (want[0].size - 1, want[3].size, want[4].size, want[7].size)
            for k, name in enumerate(NAMES):
                got = structure_array(nbx, plan, k)
                assert got.shape == want[k].shape, name
                assert np.array_equal(got, want[k]), f"N = 2^20 depth 6: {name} differs first at {int(np.nonzero(got != want[k])[0][0])}"
                want[k] = got = None


def near_refusal_bodies():
    """2^20 bodies at (i + 1/2, j + 1/2), 0 <= i, j < 1024: one per cell of a 1024^2 grid over their bounding box."""
    i = np.arange(1024, dtype=np.float64) + 0.5
    b = np.zeros((1 << 20, 5))
    b[:, 0] = np.repeat(i, 1024)
    b[:, 1] = np.tile(i, 1024)
    b[:, 4] = 1.0
    return b


def near_entries_lower_bound(b, depth, theta):
    """A lower bound on the near entries of near_refusal_bodies at (depth, theta), from the host builder's cell expression and
    the acceptance test alone.  The root box is the bounding box padded by 1 %, so at depth 10 the grid's outermost five cells per
    side stay empty and the bodies fill a contiguous m x m block of leaves (spacing 1 < cell width 1.009: no cell is skipped).
    A leaf p with |dx|, |dy| <= r cells from q has a box gap of at most (r - 1) sqrt(2); while theta (r - 1) sqrt(2) <= 1 the
    leaf-level test 1 < theta gap fails, and no ancestor of p can have been accepted either (its gap is not larger, its side is):
    p is on q's near list.  Every q at least r cells inside the block therefore has >= (2 r + 1)^2 near leaves."""
    g = 1 << depth
    origin, side = octree_inputs._root_box(b[:, :2])
    cell = np.clip(np.floor((b[:, :2] - origin) / side * g).astype(np.int64), 0, g - 1)
    cx, cy = np.unique(cell[:, 0]), np.unique(cell[:, 1])
    m = cx.size
    assert cy.size == m and cx[-1] - cx[0] == m - 1 and cy[-1] - cy[0] == m - 1, "the occupied leaves are not a full contiguous block"
    assert np.unique(cell[:, 0] * g + cell[:, 1]).size == m * m
    r = 35
    assert theta * (r - 1) * math.sqrt(2.0) < 1.0
    return m, (m - 2 * r - 2) ** 2 * (2 * r + 1) ** 2


def full_grid_bodies(dim, depth):
    """One body at the centre of every cell of a 2^depth grid: (i + 1/2, ...)."""
    i = np.arange(1 << depth, dtype=np.float64) + 0.5
    pos = np.array(np.meshgrid(*[i] * dim, indexing="ij")).reshape(dim, -1).T
    b = np.zeros((pos.shape[0], 2 * dim + 1))
    b[:, :dim] = pos
    b[:, -1] = 1.0
    return b


def full_grid_list_lengths(dim, depth, theta, chunk=1024):
    """(near entries, far entries) of the tree in which EVERY cell of the 2^depth grid is a leaf, by a count-only walk on integers
    with leaves.octree_cells's acceptance expression.  The tree of a full grid maps onto itself under the mirror q -> 2^depth - 1 - q
    of any axis and under any permutation of the axes, so only the targets with q_0 <= q_1 <= ... < 2^(depth - 1) are walked (45,760
    of 2,097,152 in 3D at depth 7), each counted with the size of its class."""
    g = 1 << depth
    reps = np.array(np.meshgrid(*[np.arange(g // 2)] * dim, indexing="ij")).reshape(dim, -1).T
    reps = reps[np.all(np.diff(reps, axis=1) >= 0, axis=1)]
    distinct = np.array([len(set(r)) for r in reps.tolist()])
    orders = np.where(distinct == 3, 6, np.where(distinct == 2, 3, 1)) if dim == 3 else np.where(distinct == 2, 2, 1)
    mult = (1 << dim) * orders
    assert int(mult.sum()) == g ** dim
    kids = np.array(np.meshgrid(*[np.arange(2)] * dim, indexing="ij")).reshape(dim, -1).T
    near_total = far_total = 0
    for c0 in range(0, reps.shape[0], chunk):
        q = reps[c0:c0 + chunk]
        k = q.shape[0]
        t, node = np.repeat(np.arange(k), kids.shape[0]), np.tile(kids, (k, 1))
        near, far = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
        for L in range(1, depth + 1):
            s_ = depth - L
            blo = node << s_
            gap = np.maximum(0, np.maximum(blo - (q[t] + 1), q[t] - (blo + (1 << s_))))
            acc = float(1 << s_) < theta * np.sqrt((gap * gap).sum(axis=1).astype(np.float64))
            far += np.bincount(t[acc], minlength=k)
            t, node = t[~acc], node[~acc]
            if L == depth:
                near += np.bincount(t, minlength=k)
            else:
                node = (node[:, None, :] * 2 + kids[None, :, :]).reshape(-1, dim)
                t = np.repeat(t, kids.shape[0])
        near_total += int((near * mult[c0:c0 + chunk]).sum())
        far_total += int((far * mult[c0:c0 + chunk]).sum())
    return near_total, far_total


def refusal_child(which, out_path):
    """Runs in a process of its own (the two tests below give it a time limit): a build whose near (far) lists pass 2^32 entries."""
    import nbody_amd as nbx
    b, dim, depth, theta, small = (near_refusal_bodies(), 2, 10, 0.02, 5) if which == "near" else (full_grid_bodies(3, 7), 3, 7, 0.5, 3)
    n = b.shape[0]
    res = {}
    with nbx.Context(n, dim) as c:
        c.upload(b)
        with nbx.LeafPlan.from_octree(c, small, 0.5) as plan:    # the first build of the process pays for the allocations
            res["sizes_before"] = plan.structure_sizes()
        t0 = time.perf_counter()
        try:
            nbx.LeafPlan.from_octree(c, depth, theta).close()
            res["status"], res["text"] = 0, ""
        except nbx.NbxError as e:
            res["status"], res["text"] = e.status, str(e)
        res["refused_build_s"] = time.perf_counter() - t0
        if which == "near":
            t0 = time.perf_counter()
            with nbx.LeafPlan.from_octree(c, depth, 100.0) as plan:  # the same tree with the shortest lists, whole build, for scale
                res["same_tree_short_lists_s"] = time.perf_counter() - t0
                res["same_tree_short_lists_sizes"] = plan.structure_sizes()
        want = nbx.leaves.octree_cells(b, dim, small, 0.5)
        with nbx.LeafPlan.from_octree(c, small, 0.5) as plan:
            assert_same_structure(plan.structure(), want, "a valid build after the refusal")
            res["valid_after"] = True
    with open(out_path, "w") as f:
        json.dump(res, f)


def run_refusal_child(which, tmp_path, limit):
    out = str(tmp_path / "refusal.json")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + [q for q in os.environ.get("PYTHONPATH", "").split(os.pathsep) if q]))
    p = subprocess.run([sys.executable, "-c", f"import test_gpu_octree_sweep as t; t.refusal_child({which!r}, {out!r})"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=limit)
    assert p.returncode == 0, p.stdout + p.stderr
    with open(out) as f:
        return json.load(f)


def test_near_lists_beyond_2_32_entries_are_refused(nbx, tmp_path):
    """One body per cell of a 1024^2 grid, 2D, depth 10, theta = 0.02: more than 2^32 near entries, which uint32 offsets cannot
    hold.  Only the counting walk runs; the build is refused with NBX_ERR_INVALID ("near lists too long") and the context builds
    a valid tree afterwards.  The host builder cannot be run on this input; the count's lower bound comes from the formula.
    Measured on an MI355X: the refused build 409 ms, against 4.4 ms for a whole build of the same tree with the shortest lists
    (theta 100): the counting walk of these lists takes 0.40 s."""
    b = near_refusal_bodies()
    m, bound = near_entries_lower_bound(b, 10, 0.02)
    print(f"\n{m} x {m} occupied leaves; at least {bound} = {bound / 2.0 ** 32:.3f} x 2^32 near entries")
    assert bound > 1 << 32 and bound > 0xfffffff0
    # sized from the depth-6 record (profiles/r7/octree_device.txt): 3.3 ms for 256,791 lanes of ~2,500 tested nodes each is
    # 2e11 tests / s; here 1,028,196 lanes test ~15,000 nodes each (8,200 leaves within a gap of 50, their ancestors, the accepted
    # ring): 1.5e10 tests, 0.1 s at that rate and seconds if the long divergent walks run ten times worse.  300 s covers the
    # process, three other builds and the host builder at depth 5.
    res = run_refusal_child("near", tmp_path, 300)
    print(f"refused build (tree + counting walk) {res['refused_build_s'] * 1e3:.1f} ms; the same tree at theta 100, whole build "
          f"{res['same_tree_short_lists_s'] * 1e3:.1f} ms {res['same_tree_short_lists_sizes']}")
    assert res["status"] == NBX_ERR_INVALID and "near lists too long" in res["text"], res
    assert res["same_tree_short_lists_sizes"][0] == m * m
    assert res["valid_after"]


def test_far_lists_beyond_2_32_entries_are_refused(nbx, tmp_path):
    """One body per cell of a 128^3 grid, 3D, depth 7, theta = 0.5: 5.27e9 far entries (and 3.6e8 near entries, which fit).  The
    count comes from full_grid_list_lengths, which is first held against the host builder where that can run (3D depth 3 and 4,
    2D depth 5).  The build is refused with NBX_ERR_INVALID ("far lists too long"); a valid build follows on the same context.
    Measured on an MI355X: the refused build (tree and counting walk) 26 ms."""
    for dim, depth in ((3, 3), (3, 4), (2, 5)):
        want = nbx.leaves.octree_cells(full_grid_bodies(dim, depth), dim, depth, 0.5)
        assert want[0].size - 1 == 1 << (dim * depth)
        assert full_grid_list_lengths(dim, depth, 0.5) == (want[3].size, want[7].size), (dim, depth)
    b = full_grid_bodies(3, 7)
    assert octree_inputs.leaf_count(nbx.leaves, b, 3, 7) == b.shape[0] == 1 << 21, "not every cell of the root box's grid holds one body"
    near, far = full_grid_list_lengths(3, 7, 0.5)
    print(f"\n128^3 leaves: {near} near entries, {far} = {far / 2.0 ** 32:.3f} x 2^32 far entries")
    assert far > 1 << 32 and near <= 0xfffffff0
    # 2,097,152 lanes of ~3,000 tested nodes: 6e9 tests, 0.03 s at the depth-6 record's rate
    res = run_refusal_child("far", tmp_path, 300)
    print(f"refused build (tree + counting walk) {res['refused_build_s'] * 1e3:.1f} ms")
    assert res["status"] == NBX_ERR_INVALID and "far lists too long" in res["text"], res
    assert res["valid_after"]
