"""CPU: the host side of a leaf plan's far field -- the structure builder leaves.octree_cells, the null-plan refusals of the three
nbx_leaf_plan_*cells entry points (no device needed), and csrc/leaf_far.h (validation of the caller's arrays and the cutting of the
far pass's waves) compiled with g++ under ASan / UBSan, the way tests/test_leaf_plan_cpu.py runs csrc/leaf_plan.h."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bodies(seed, n, dim):
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 2 * dim + 1))
    b[:, :dim] = rng.uniform(1.0, 1.0e7, (n, dim))
    b[:, -1] = rng.uniform(1.0, 1.0e8, n)
    return b


def _morton_of_bodies(b, dim, depth):
    """Z-order key of every body's grid cell, restated here: the bits of the axes interleaved, axis 0 the most significant of a level."""
    pos = b[:, :dim]
    g = 1 << depth
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    origin, side = (lo + hi) / 2.0 - (hi - lo).max() / 2.0 * 1.01, (hi - lo).max() * 1.01
    cell = np.clip(np.floor((pos - origin) / side * g).astype(np.int64), 0, g - 1)
    keys = []
    for c in cell:
        bits = "".join("".join(format(int(c[d]), f"0{depth}b")[level] for d in range(dim)) for level in range(depth))
        keys.append(int(bits, 2) if bits else 0)
    return np.array(keys, dtype=np.int64)


@pytest.mark.parametrize("theta", (0.0, 0.3, 0.5, 1.0))
@pytest.mark.parametrize("dim,depth", ((2, 1), (2, 3), (2, 5), (3, 1), (3, 2), (3, 4)))
def test_octree_cells_cover_every_leaf_exactly_once(nbx, dim, depth, theta):
    n = 3000
    b = _bodies(10 * dim + depth, n, dim)
    lo, lb, so, ss, cf, cc, fo, fc = (a.astype(np.int64) for a in nbx.leaves.octree_cells(b, dim, depth, theta, chunk_leaves=97))
    nl = lo.size - 1
    assert lo[0] == 0 and lo[-1] == n and (np.diff(lo) > 0).all() and np.array_equal(np.sort(lb), np.arange(n))
    assert so.size == nl + 1 and fo.size == nl + 1 and so[-1] == ss.size and fo[-1] == fc.size
    # Morton order: every body's key equals its leaf's, leaf keys strictly increase
    key = _morton_of_bodies(b, dim, depth)
    leaf_key = key[lb[lo[:-1]]]
    assert (np.diff(leaf_key) > 0).all()
    assert np.array_equal(np.repeat(leaf_key, np.diff(lo)), key[lb])
    # cells: the non-empty nodes of levels 1 .. depth, each the contiguous range of its descendants
    want = sum(np.unique(leaf_key >> (dim * (depth - L))).size for L in range(1, depth + 1))
    assert cf.size == want and (cc >= 1).all() and (cf + cc <= nl).all()
    at = 0
    for L in range(1, depth + 1):
        node = leaf_key >> (dim * (depth - L))
        u, first, count = np.unique(node, return_index=True, return_counts=True)
        assert np.array_equal(cf[at:at + u.size], first) and np.array_equal(cc[at:at + u.size], count)
        at += u.size
    assert np.array_equal(cf[-nl:], np.arange(nl)) and (cc[-nl:] == 1).all()       # the last level: the leaves themselves
    for t in range(nl):
        near, far = ss[so[t]:so[t + 1]], fc[fo[t]:fo[t + 1]]
        assert near.size and near[0] == t, "the leaf itself first"
        seen = np.bincount(near, minlength=nl)
        for c in far:
            seen[cf[c]:cf[c] + cc[c]] += 1
        assert (seen == 1).all(), f"leaf {t}: near leaves and far cells must cover every leaf exactly once"
    if theta == 0.0:
        assert fc.size == 0 and (np.diff(so) == nl).all(), "theta = 0: every leaf is near"
    elif depth >= 3:
        assert fc.size > 0


def test_octree_cells_acceptance_is_the_box_gap_test(nbx):
    """Every accepted cell is farther from the target leaf's box than side / theta (box to box)."""
    dim, depth, theta = 3, 3, 0.5
    b = _bodies(5, 4000, dim)
    lo, lb, so, ss, cf, cc, fo, fc = (a.astype(np.int64) for a in nbx.leaves.octree_cells(b, dim, depth, theta))
    pos = b[:, :dim]
    for t in range(0, lo.size - 1, 17):
        mine = pos[lb[lo[t]:lo[t + 1]]]
        for c in fc[fo[t]:fo[t + 1]]:
            theirs = pos[lb[lo[cf[c]]:lo[cf[c] + cc[c]]]]
            ext = float(np.ptp(theirs, axis=0).max())
            d = np.sqrt(((mine[:, None, :] - theirs[None, :, :]) ** 2).sum(axis=2)).min()
            assert d > ext / theta


@pytest.mark.parametrize("n", (0, 1))
def test_octree_cells_of_nothing_and_of_one_body(nbx, n):
    b = _bodies(1, n, 3)
    lo, lb, so, ss, cf, cc, fo, fc = nbx.leaves.octree_cells(b, 3, 3, 0.5)
    assert all(a.dtype == np.uint32 for a in (lo, lb, so, ss, cf, cc, fo, fc))
    if n == 0:
        assert lo.tolist() == [0] and so.tolist() == [0] and fo.tolist() == [0] and not (lb.size or ss.size or cf.size or cc.size or fc.size)
    else:
        assert lo.tolist() == [0, 1] and lb.tolist() == [0] and ss.tolist() == [0] and fo.tolist() == [0, 0]
        assert cf.tolist() == [0, 0, 0] and cc.tolist() == [1, 1, 1]


def test_cell_entries_reject_a_null_plan(nbx):
    lib = nbx.load_library()
    assert lib.nbx_leaf_plan_set_cells(None, None, None, 0, None, None) == 1
    assert lib.nbx_leaf_plan_get_cells(None, None, None) == 1
    assert lib.nbx_leaf_plan_cell_info(None, None, None, None, None) == 1
    assert b"plan is null" in lib.nbx_last_error_detail()


def test_far_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "leaf_far_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + ROOT,
           os.path.join(ROOT, "tests", "leaf_far_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout
