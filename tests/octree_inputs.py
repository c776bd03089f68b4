"""Named inputs for the octree builders (test infrastructure; used by tests/test_octree_build_cpu.py, which runs them through the
g++ build of csrc/octree_device.h, and by tests/test_gpu_octree_sweep.py, which runs the same bodies through the device builder).

Every generator is  f(oracle, dim, n, seed, depth) -> bodies [n, 2 dim + 1]  (positions, velocities, mass), deterministic from
its arguments.  The positions are rounded to fp32 like every other GPU input, EXCEPT where rounding would destroy what the input
is for: `planes` (fp64 positions on the root box's grid planes and one fp64 ulp off them) and `denormal` (multiples of 5e-324).
The builders read the context's resident fp64 positions, so both are legitimate inputs.  `depth` matters to `lattice` and `planes`
only (their grids are the tree's); the others ignore it.

Also here: the host-side self-checks of the inputs (share of bodies on a grid plane, exact ties of the acceptance test), all
computed with the host builder's own expressions and evaluated before any device result is looked at."""
import numpy as np


def _root_box(pos):
    """origin, side of leaves.octree_cells's root box."""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    centre, half = (lo + hi) / 2.0, max(float((hi - lo).max()) / 2.0 * 1.01, 1e-300)
    return centre - half, 2.0 * half


def _bodies(pos, dim):
    b = np.zeros((pos.shape[0], 2 * dim + 1))
    b[:, :dim] = pos
    b[:, -1] = 1.0
    return b


def uniform(oracle, dim, n, seed, depth=None):
    """The reference generator's bodies: positive coordinates, uniform in a cube."""
    return oracle.round_inputs_to_f32(oracle.generate(seed, n, dim))


def signed(oracle, dim, n, seed, depth=None):
    """uniform - 5e6: every combination of signs occurs, and the root box straddles the origin."""
    b = oracle.generate(seed, n, dim)
    b[:, :dim] -= 5.0e6
    return oracle.round_inputs_to_f32(b)


def tiny(oracle, dim, n, seed, depth=None):
    b = oracle.generate(seed, n, dim)
    b[:, :dim] *= 1.0e-30
    return oracle.round_inputs_to_f32(b)


def huge(oracle, dim, n, seed, depth=None):
    """Coordinates up to 1e37: in fp32's range, and hi - lo is 270 orders of magnitude below fp64's overflow."""
    b = oracle.generate(seed, n, dim)
    b[:, :dim] *= 1.0e30
    return oracle.round_inputs_to_f32(b)


def slab(oracle, dim, n, seed, depth=None):
    """z constant: the widest axis decides the box, the last axis has zero extent and sits on the box's mid plane."""
    assert dim == 3
    b = oracle.generate(seed, n, dim)
    b[:, 2] = b[0, 2]
    return oracle.round_inputs_to_f32(b)


def line(oracle, dim, n, seed, depth=None):
    assert dim == 3
    b = oracle.generate(seed, n, dim)
    b[:, 1:3] = b[0, 1:3]
    return oracle.round_inputs_to_f32(b)


def lattice(oracle, dim, n, seed, depth):
    """Integer coordinates 0 .. g inclusive, g = 2^depth, many bodies per site (n >> the sites drawn).  The root box is the
    lattice's box padded by 1 %, so its cells are 1.01 wide and the ONE lattice plane that coincides with a grid plane is the mid
    plane x = g / 2 (the box is centred on it).  Per axis a quarter of the draws are g / 2, the rest uniform over 0 .. g: in 3D
    1 - (3/4)^3 = 58 % of the bodies (2D: 44 %) have a coordinate on that plane.  The two corner sites keep the box as it is."""
    g = 1 << depth
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, g + 1, (n, dim)).astype(np.float64)
    pos[rng.random((n, dim)) < 0.25] = g / 2.0
    if n >= 2:
        pos[0], pos[1] = 0.0, float(g)
    return oracle.round_inputs_to_f32(_bodies(pos, dim))


def plane_positions(dim, depth, seed, n_on=3000, n_face=100):
    """Positions exactly on the grid planes of the root box (and one ulp to either side), and on the faces of the bounding box:
    two corners that fix the box, n_on bodies on planes in every axis, their two neighbours, 2 dim n_face bodies on faces."""
    g = 1 << depth
    corners = np.array([[1.0] * dim, [1.0e7] * dim])
    origin, side = _root_box(corners)
    rng = np.random.default_rng(seed)
    k = rng.integers(1, g, (n_on, dim))
    on = origin + side * (k / g)
    on = np.clip(on, 1.0, 1.0e7)                                     # the two corners keep the box as it is
    pos = np.concatenate([corners, on, np.nextafter(on, -np.inf), np.nextafter(on, np.inf)])
    faces = rng.uniform(1.0, 1.0e7, (6 * n_face, dim))
    for d in range(dim):
        faces[2 * n_face * d:2 * n_face * d + n_face, d] = 1.0                        # on the lower face of the bounding box ...
        faces[2 * n_face * d + n_face:2 * n_face * (d + 1), d] = 1.0e7                # ... and on the upper one
    return np.concatenate([pos, faces[:2 * n_face * dim]])


def planes(oracle, dim, n, seed, depth):
    """plane_positions as bodies: about n of them (a third on planes, a third each one ulp below and above, 6 % on faces)."""
    n_face = max(1, n // (100 * dim))
    return _bodies(plane_positions(dim, depth, seed, n_on=(n - 2 - 2 * dim * n_face) // 3, n_face=n_face), dim)


def duplicates(oracle, dim, n, seed, depth=None):
    """uniform with 30 % of the bodies copied onto others: equal keys from equal positions, in runs the stable sort must keep."""
    b = uniform(oracle, dim, n, seed)
    rng = np.random.default_rng(seed)
    to = rng.choice(n, (3 * n) // 10, replace=False)
    b[to, :dim] = b[rng.integers(0, n, to.size), :dim]
    return b


def one_point(oracle, dim, n, seed, depth=None):
    b = oracle.round_inputs_to_f32(oracle.generate(seed, n, dim))
    b[:, :dim] = b[0, :dim]
    return b


def denormal(oracle, dim, n, seed, depth=None):
    """Coordinates 0 .. 7 x 5e-324: the half side hits the floor of 1e-300 and every body lands in one leaf."""
    rng = np.random.default_rng(seed)
    return _bodies(rng.integers(0, 8, (n, dim)) * 5e-324, dim)


def clustered(oracle, dim, n, seed, depth=None):
    """Two Gaussian blobs of n / 2 bodies each: leaves of hundreds of bodies next to empty octants."""
    b = oracle.generate(seed, n, dim)
    rng = np.random.default_rng(seed)
    scale = float(np.abs(b[:, :dim]).max())
    h = n // 2
    b[:h, :dim] = rng.normal(-0.4 * scale, 0.001 * scale, size=(h, dim))
    b[h:, :dim] = rng.normal(0.3 * scale, 0.05 * scale, size=(n - h, dim))
    return oracle.round_inputs_to_f32(b)


GENERATORS = {f.__name__: f for f in (uniform, signed, tiny, huge, slab, line, lattice, planes, duplicates, one_point, denormal, clustered)}

# Radix passes of the device builder's key sort: ceil(dim depth / 8).
def passes(dim, depth):
    return (dim * depth + 7) // 8


# (generator, dim, n, seed, depths): every generator at a depth with an even and one with an odd pass count -- 3D: depth 4
# (12 bits, 2 passes) and 7 (21 bits, 3); 2D: depth 6 (12 bits, 2) and 4 (8 bits, 1) -- in 3D and, where the input exists there,
# in 2D.  One point also at the depths it had before (3) and the deepest (10).  The CPU twin and the GPU sweep run the same list.
GEOMETRY_CASES = tuple(
    [(name, 3, 20000, 400 + i, (4, 7)) for i, name in enumerate(("uniform", "signed", "tiny", "huge", "slab", "line", "lattice", "planes", "duplicates", "denormal"))]
    + [(name, 2, 20000, 420 + i, (6, 4)) for i, name in enumerate(("signed", "tiny", "huge", "lattice", "planes", "duplicates", "denormal"))]
    + [("one_point", 3, 1000, 92, (3, 7, 10)), ("one_point", 2, 1000, 92, (6, 4)), ("clustered", 3, 60000, 91, (4, 7)), ("clustered", 2, 60000, 91, (6, 4))])
for _name, _dim, _n, _seed, _depths in GEOMETRY_CASES:
    assert {passes(_dim, d) % 2 for d in _depths} == {0, 1}, (_name, _dim, _depths)
assert {c[0] for c in GEOMETRY_CASES} == set(GENERATORS)


# Body counts on both sides of the builder's tile edges: 64 (leaves per walk workgroup, bodies per far block), 256 (threads per
# block), 2,048 (scan tile), 4,096 (sort tile), 65,536 (the bounding box's stride).  Each runs in 3D at depth 3 (9 key bits, 2
# passes; at most 512 leaves) and at depth 6 (18 bits, 3 passes; 262,144 cells, so the leaf count follows n across 64 and 256).
SIZES = (2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537)
SIZE_DEPTHS = (3, 6)
assert [passes(3, d) for d in SIZE_DEPTHS] == [2, 3]


def size_case(oracle, n):
    return uniform(oracle, 3, n, 500 + SIZES.index(n))


def leaf_count(leaves, bodies, dim, depth):
    """n_leaves of leaves.octree_cells without its lists: the distinct keys of the host builder's cells."""
    pos = np.asarray(bodies)[:, :dim]
    g = 1 << depth
    origin, side = _root_box(pos)
    cell = np.clip(np.floor((pos - origin) / side * g).astype(np.int64), 0, g - 1)
    return int(np.unique(leaves._morton_keys(cell, dim, depth)).size)


def share_on_grid_planes(pos, depth):
    """The share of bodies with a coordinate exactly on an inner grid plane of the root box, by the host builder's own expression:
    (x - origin) / side * 2^depth comes out a whole number strictly between 0 and 2^depth in at least one axis."""
    g = 1 << depth
    origin, side = _root_box(pos)
    t = (pos - origin) / side * g
    return float(np.any((t == np.floor(t)) & (t > 0) & (t < g), axis=1).mean())


def count_exact_ties(leaves, bodies, dim, depth, theta, chunk_leaves=1024):
    """The (target leaf, node) pairs that the walk of leaves.octree_cells TESTS and whose test ties exactly: 2^s == theta *
    sqrt(sum of squared gaps) in the builder's own fp64 expression.  The builder's level-synchronous walk is repeated here on
    integers alone (a node is tested when its parent was tested and not accepted; a tie is not accepted).  `leaves`: the module."""
    pos = np.asarray(bodies)[:, :dim]
    g = 1 << depth
    origin, side = _root_box(pos)
    cell = np.clip(np.floor((pos - origin) / side * g).astype(np.int64), 0, g - 1)
    keys = np.unique(leaves._morton_keys(cell, dim, depth))
    q = leaves._morton_coords(keys, dim, depth)
    level = {L: np.unique(keys >> (dim * (depth - L))) for L in range(1, depth + 1)}
    coords = {L: leaves._morton_coords(level[L], dim, L) for L in level}
    ties = 0
    for t0 in range(0, keys.size, chunk_leaves):
        t1 = min(keys.size, t0 + chunk_leaves)
        t = np.repeat(np.arange(t0, t1, dtype=np.int64), level[1].size)
        node = np.tile(np.arange(level[1].size, dtype=np.int64), t1 - t0)
        for L in range(1, depth + 1):
            s = depth - L
            blo = coords[L][node] << s
            gap = np.maximum(0, np.maximum(blo - (q[t] + 1), q[t] - (blo + (1 << s))))
            reach = theta * np.sqrt((gap * gap).sum(axis=1).astype(np.float64))
            ties += int((float(1 << s) == reach).sum())
            keep = ~(float(1 << s) < reach)
            t, node = t[keep], node[keep]
            if L == depth:
                break
            first = np.searchsorted(level[L + 1], level[L][node] << dim)
            cnt = np.searchsorted(level[L + 1], (level[L][node] + 1) << dim) - first
            start = np.repeat(np.cumsum(cnt) - cnt, cnt)
            t, node = np.repeat(t, cnt), np.repeat(first, cnt) + (np.arange(int(cnt.sum()), dtype=np.int64) - start)
    return ties
