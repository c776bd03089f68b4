"""CPU: the one definition of the root box, the cell index and the Morton key that the device builder (csrc/octree_device.hip)
compiles for the GPU, compiled here with g++ -ffp-contract=off under ASan / UBSan (tests/octree_key_check.cpp), against the host
builder: the keys equal leaves._morton_keys of the host's cells, and their stable argsort equals leaves.octree_cells's body
order.  Also the null-argument refusals of the new entry points, which need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import octree_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def key_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("octree_key_check") / "octree_key_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + ROOT,
           os.path.join(ROOT, "tests", "octree_key_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return str(exe)


def host_cells(pos, dim, depth):
    """The cell of every body, as leaves.octree_cells computes it."""
    g = 1 << depth
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre, half = (lo + hi) / 2.0, max(float((hi - lo).max()) / 2.0 * 1.01, 1e-300)
    return np.clip(np.floor((pos - (centre - half)) / (2.0 * half) * g).astype(np.int64), 0, g - 1), centre - half, 2.0 * half


def compare(nbx, key_check, tmp_path, pos, dim, depth, what):
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = pos.shape[0]
    src, dst = str(tmp_path / "in.f64"), str(tmp_path / "out.u32")
    np.concatenate([[float(n), float(dim), float(depth)], pos.ravel()]).tofile(src)
    p = subprocess.run([key_check, src, dst], capture_output=True, text=True)
    assert p.returncode == 0, what + ": " + p.stdout + p.stderr
    got = np.fromfile(dst, dtype=np.uint32).astype(np.int64)
    cell, _, _ = host_cells(pos, dim, depth)
    want = nbx.leaves._morton_keys(cell, dim, depth)
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {n} keys differ"
    b = np.zeros((n, 2 * dim + 1))
    b[:, :dim] = pos
    b[:, -1] = 1.0
    assert np.array_equal(np.argsort(got, kind="stable").astype(np.uint32), nbx.leaves.octree_cells(b, dim, depth, 0.5)[1]), what
    return cell


@pytest.mark.parametrize("dim,depth", ((2, 0), (2, 4), (2, 10), (3, 0), (3, 3), (3, 10)))
def test_keys_of_random_bodies(nbx, key_check, tmp_path, dim, depth):
    rng = np.random.default_rng(100 * dim + depth)
    pos = rng.uniform(1.0, 1.0e7, (4000, dim))
    pos[:1000] = np.float32(pos[:1000])                              # the rounded inputs the GPU tests use
    compare(nbx, key_check, tmp_path, pos, dim, depth, f"random dim {dim} depth {depth}")


@pytest.mark.parametrize("dim,depth", ((2, 5), (3, 4), (3, 10)))
def test_keys_on_cell_boundaries_and_box_faces(nbx, key_check, tmp_path, dim, depth):
    """Bodies exactly on the grid planes of the root box (and one ulp to either side), and on the faces of the bounding box."""
    pos = octree_inputs.plane_positions(dim, depth, 7 * dim + depth)
    assert pos.shape[0] == 2 + 3 * 3000 + 200 * dim
    assert octree_inputs.share_on_grid_planes(pos, depth) >= 1.0 / 3.0, "the input misses the planes it is made for"
    compare(nbx, key_check, tmp_path, pos, dim, depth, f"boundaries dim {dim} depth {depth}")


@pytest.mark.parametrize("dim", (2, 3))
def test_keys_of_a_single_point(nbx, key_check, tmp_path, dim):
    """Every body at one point: the box's half side is the floor of 1e-300."""
    for n in (1, 500):
        for depth in (0, 4, 10):
            pos = np.tile(np.array([[3.25e6, 1.0, 9.9e6]])[:, :dim], (n, 1))
            compare(nbx, key_check, tmp_path, pos, dim, depth, f"{n} bodies at one point, depth {depth}")
    compare(nbx, key_check, tmp_path, np.zeros((10, dim)), dim, 3, "bodies at the origin")
    compare(nbx, key_check, tmp_path, -np.abs(np.random.default_rng(5).normal(0, 1e-3, (300, dim))), dim, 6, "small negative coordinates")


GEOMETRY = [(name, dim, n, seed, depth) for name, dim, n, seed, depths in octree_inputs.GEOMETRY_CASES for depth in depths]


@pytest.mark.parametrize("name,dim,n,seed,depth", GEOMETRY, ids=[f"{c[0]}-{c[1]}d-depth{c[4]}" for c in GEOMETRY])
def test_keys_of_every_named_input(nbx, oracle, key_check, tmp_path, name, dim, n, seed, depth):
    """The CPU twin of tests/test_gpu_octree_sweep.py's geometry cases: the same bodies at the same depths through the g++ build of
    the shared header.  A device mismatch on one of them that this test does not show lies in the device kernels, not the header."""
    b = octree_inputs.GENERATORS[name](oracle, dim, n, seed, depth)
    assert b.shape[1] == 2 * dim + 1 and abs(b.shape[0] - n) <= 2 * dim + 2
    if name in ("planes", "lattice"):
        assert octree_inputs.share_on_grid_planes(b[:, :dim], depth) >= 1.0 / 3.0, "the input misses the planes it is made for"
    cell = compare(nbx, key_check, tmp_path, b[:, :dim], dim, depth, f"{name} dim {dim} depth {depth}")
    if name in ("one_point", "denormal"):
        assert np.unique(cell, axis=0).shape[0] == 1                 # everything in one leaf
    if name in ("slab", "line"):
        assert np.unique(cell[:, 2]).size == 1 and np.unique(cell[:, 0]).size > 1


def test_size_cases_put_leaf_counts_on_the_wave_edges(nbx, oracle):
    """The body counts of the GPU size sweep (octree_inputs.SIZES, with their seeds) give, by the host builder alone, leaf counts
    that are 0, 1 and 63 mod 64: a full last wave of the walk, a wave of one lane, and a wave one lane short."""
    counts = {(n, depth): octree_inputs.leaf_count(nbx.leaves, octree_inputs.size_case(oracle, n), 3, depth)
              for n in octree_inputs.SIZES for depth in octree_inputs.SIZE_DEPTHS}
    print("\n" + "\n".join(f"n {n} depth {depth}: n_leaves {nl} (mod 64: {nl % 64}, mod 256: {nl % 256})" for (n, depth), nl in counts.items()))
    assert {nl % 64 for nl in counts.values()} >= {0, 1, 63}
    assert {nl % 256 for nl in counts.values()} >= {0, 1, 255}


def test_octree_entries_reject_null_arguments(nbx):
    lib = nbx.load_library()
    h = ctypes.c_void_p()
    assert lib.nbx_leaf_plan_create_octree(None, None, 3, 0.5) == 1
    assert lib.nbx_leaf_plan_create_octree(ctypes.byref(h), None, 3, 0.5) == 1 and not h.value
    assert b"null" in lib.nbx_last_error_detail()
    assert lib.nbx_leaf_plan_rebuild_octree(None, None) == 1
    assert lib.nbx_leaf_plan_structure_sizes(None, None, None, None, None) == 1
    assert lib.nbx_leaf_plan_get_structure(None, None, None, None, None, None, None, None, None) == 1
    assert lib.nbx_leaf_plan_step_octree(None, None, 1, 1.0, 1.0, 1, 1) == 1
