"""CPU: the one definition of the root box, the cell index and the Morton key that the device builder (csrc/octree_device.hip)
compiles for the GPU, compiled here with g++ -ffp-contract=off under ASan / UBSan (tests/octree_key_check.cpp), against the host
builder: the keys equal leaves._morton_keys of the host's cells, and their stable argsort equals leaves.octree_cells's body
order.  Also the null-argument refusals of the new entry points, which need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

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
    g = 1 << depth
    corners = np.array([[1.0] * dim, [1.0e7] * dim])
    _, origin, side = host_cells(corners, dim, depth)
    rng = np.random.default_rng(7 * dim + depth)
    k = rng.integers(1, g, (3000, dim))
    on = origin + side * (k / g)
    on = np.clip(on, 1.0, 1.0e7)                                     # the two corners keep the box as it is
    pos = np.concatenate([corners, on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)])
    faces = rng.uniform(1.0, 1.0e7, (600, dim))
    for d in range(dim):
        faces[200 * d:200 * d + 100, d] = 1.0                        # on the lower face of the bounding box ...
        faces[200 * d + 100:200 * d + 200, d] = 1.0e7                # ... and on the upper one
    pos = np.concatenate([pos, faces[:200 * dim]])
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
