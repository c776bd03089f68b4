"""GPU: the C ABI's layout promises beyond the one layout every other test feeds it.

  - WIDER BODY RECORDS.  include/nbody_hip.h: body_stride_bytes = sizeof(Body<dim>) "(56 or 40; larger strides allowed)".  Every
    entry point that takes a stride is fed (n, 2D+1+e) records whose extra columns hold NaN, 1e20 (read as a mass it flips the fast
    path's kFastMaxMass precondition, read as a coordinate kOneRcpMaxCoord) and -0.0, and must give the bits of the same call at the
    minimal stride -- a path the rest of the suite already pins to the oracle -- while leaving every column it does not own as it was.
    A stride below sizeof(Body<dim>) or not a multiple of 8 is NBX_ERR_INVALID, with the caller's output untouched and the context,
    plan or node still usable.
  - EMPTY AND ONE-BODY SHARDS.  nbx_ctx_create gives shard g no bodies when g * shard_len >= N; every pass, the mixed mode's
    bookkeeping, the energy and the exports must hold for such partitions (N = 5 on 8 ranks, N = 0, ...) and for shards on and
    just past the 4096-body pad quantum.
  - RAW ACCELERATIONS.  nbx_ctx_get_accel writes float[dim][count]: the fp32 rounding of the sums nbx_ctx_get_forces scales by
    -(G m), for every variant, precision mode and law.
The Python wrappers accept only the minimal layout, so the wide calls go through ctypes (nbx.load_library()) directly."""
import ctypes

import numpy as np
import pytest

import cross_shard_case as csc
from oracle_lib import assert_force_parity
from test_gpu_leaf_pairs import planner
from test_gpu_strict import _assert_strict

pytestmark = pytest.mark.gpu

NBX_ERR_INVALID, NBX_ERR_STATE = 1, 5
SENTINELS = (np.nan, 1.0e20, -0.0)


def _min_stride(dim):
    return (2 * dim + 1) * 8


def _strides(dim):
    """min + 8 B, min + 24 B and 256 B records."""
    m = _min_stride(dim)
    return (m + 8, m + 24, 256)


def _bad_strides(dim):
    return (_min_stride(dim) - 8, 57, 0)


def _wide(b, stride):
    """b laid out in records of `stride` bytes; the extra columns hold the sentinels, each kind in every column."""
    n, w = b.shape
    cols = stride // 8
    out = np.empty((n, cols), dtype=np.float64)
    out[:, :w] = b
    for j in range(w, cols):
        out[:, j] = np.array([SENTINELS[(i + j) % 3] for i in range(n)], dtype=np.float64) if n else 0.0
    return out


def _sentinel_array(shape, dtype=np.float64):
    a = np.empty(shape, dtype=dtype)
    flat = a.reshape(-1)
    for k in range(3):
        flat[k::3] = SENTINELS[k]
    return a


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _inputs(oracle, seed, n, dim):
    return oracle.round_inputs_to_f32(oracle.generate(seed, n, dim))


def _small_coordinates(oracle, seed, n, dim):
    """Every coordinate below 16384: all bodies are close-set candidates, the fast path finds its close pairs through sorted cells."""
    rng = np.random.default_rng(seed)
    b = oracle.generate(seed, n, dim)
    b[:, :dim] = rng.normal(scale=1.0, size=(n, dim))
    b[10, :dim] = b[11, :dim]
    b[10, 0] += 4.0e-6                                      # r^2 = 1.6e-11: skipped
    return oracle.round_inputs_to_f32(b)


def _lib(nbx):
    return nbx.load_library()


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _csr(leaves):
    return [np.ascontiguousarray(a, dtype=np.uint32) for a in leaves]


# ---- wide records ------------------------------------------------------------------------------------------------------

def _one_shot(nbx, b, stride, G, tol, dim):
    lib = _lib(nbx)
    n = b.shape[0]
    out = np.empty((n, dim))
    info = nbx.EvalInfo()
    rc = lib.nbx_brute_force_forces_ex(_ptr(b), n, dim, stride, G, 0, tol, _ptr(out), ctypes.byref(info))
    assert rc == 0, (rc, lib.nbx_last_error_detail())
    return out, (info.variant, info.close_set_mode, info.refine_selected, info.refine_refined)


@pytest.mark.parametrize("dim", (3, 2))
def test_one_shot_forces_at_wide_strides(nbx, oracle, dim):
    """nbx_brute_force_forces(_ex), plain fp32 and mixed mode, on a uniform input and on a small-coordinate one (sorted cells)."""
    lib = _lib(nbx)
    G = oracle.G
    cases = (("uniform", _inputs(oracle, 301, 3000, dim)), ("small coordinates", _small_coordinates(oracle, 302, 3000, dim)))
    for name, b in cases:
        n = b.shape[0]
        assert_force_parity(nbx.brute_force_hip_n_body(b, G), oracle.brute_force_seq(b), oracle.force_magnitude_sums(b), name)
        for tol in (0.0, 1e-5):
            ref, ref_info = _one_shot(nbx, b, _min_stride(dim), G, tol, dim)
            if name == "small coordinates":
                assert ref_info[1] == 1, f"{name}: the sorted-cells close-set path must run ({ref_info})"
            for stride in _strides(dim):
                w = _wide(b, stride)
                keep = w.copy()
                got, info = _one_shot(nbx, w, stride, G, tol, dim)
                assert _same_bits(got, ref), f"{name} D={dim} tol={tol} stride={stride}: forces differ from the minimal stride's"
                assert info == ref_info, (name, tol, stride, info, ref_info)
                assert _same_bits(w, keep), f"{name} stride={stride}: the read-only input was written"
        plain = np.empty((n, dim))
        ms = ctypes.c_float(0.0)
        ref = nbx.brute_force_hip_n_body(b, G)
        for stride in _strides(dim):
            w = _wide(b, stride)
            assert lib.nbx_brute_force_forces(_ptr(w), n, dim, stride, G, 0, _ptr(plain), ctypes.byref(ms)) == 0
            assert _same_bits(plain, ref), f"{name} stride={stride}: nbx_brute_force_forces differs"


@pytest.mark.parametrize("dim", (3, 2))
def test_leapfrog_at_wide_strides(nbx, oracle, dim):
    """nbx_leapfrog updates positions and velocities in place and nothing else: the mass column and every extra column keep their bits."""
    lib = _lib(nbx)
    n, dt, steps = 2000, 2.0, 4                              # 4 steps: the graph-replayed path
    G = oracle.G * 1e24
    b = _inputs(oracle, 303, n, dim)
    ref = b.copy()
    nbx.leapfrog_hip_n_body(ref, dt, steps, G)
    assert np.abs(ref[:, dim:2 * dim] - b[:, dim:2 * dim]).max() > 1e-6, "coupling too weak to see a misread body"
    for stride in _strides(dim):
        w = _wide(b, stride)
        keep = w.copy()
        assert lib.nbx_leapfrog(_ptr(w), n, dim, stride, G, dt, steps, 0, None) == 0
        assert _same_bits(w[:, :2 * dim], ref[:, :2 * dim]), f"stride={stride}: state differs from the minimal stride's"
        assert _same_bits(w[:, 2 * dim:], keep[:, 2 * dim:]), f"stride={stride}: mass or extra columns were written"


@pytest.mark.parametrize("dim", (3, 2))
def test_context_upload_and_download_at_wide_strides(nbx, oracle, dim):
    """nbx_ctx_upload_bodies (forces, effective tuning, close-set mode), the sharded upload nbx_ctx_upload_shard + nbx_ctx_upload_finish on
    three shards sharing one pair of exchange buffers, and nbx_ctx_download_bodies into a sentinel-filled array."""
    lib = _lib(nbx)
    G = oracle.G
    n = 3001
    for name, b in (("uniform", _inputs(oracle, 304, n, dim)), ("small coordinates", _small_coordinates(oracle, 305, n, dim))):
        with nbx.Context(n, dim) as c:
            c.upload(b)
            c.compute_accel()
            ref, ref_tune, ref_mode = c.forces(G), c.effective_tuning(), c.close_set_mode()[0]
        assert_force_parity(ref, oracle.brute_force_seq(b), oracle.force_magnitude_sums(b), name)
        for stride in _strides(dim):
            w = _wide(b, stride)
            keep = w.copy()
            with nbx.Context(n, dim) as c:
                assert lib.nbx_ctx_upload_bodies(c.h, _ptr(w), stride) == 0
                assert c.effective_tuning() == ref_tune and c.close_set_mode()[0] == ref_mode, (name, stride)
                c.compute_accel()
                assert _same_bits(c.forces(G), ref), f"{name} stride={stride}: context forces differ"
            assert _same_bits(w, keep)

    # three shards, each uploading only its own rows into exchange buffers the three contexts share (rank 0's, allocated at its upload)
    b = _inputs(oracle, 306, n, dim)
    shards = 3

    def sharded(stride):
        src = b if stride == _min_stride(dim) else _wide(b, stride)
        ctxs = [nbx.Context(n, dim, n_shards=shards, shard=r) for r in range(shards)]
        maxima, out = [], []
        try:
            for c in ctxs:
                if c.shard:
                    pos, mass = ctypes.c_void_p(), ctypes.c_void_p()
                    assert lib.nbx_ctx_gather_layout(ctxs[0].h, None, None, ctypes.byref(pos), ctypes.byref(mass)) == 0
                    c.set_gather_buffers(pos.value, mass.value)
                lo = c.shard * c.shard_len
                mine = np.ascontiguousarray(src[lo:lo + c.count])
                m, x = ctypes.c_double(0.0), ctypes.c_double(0.0)
                assert lib.nbx_ctx_upload_shard(c.h, _ptr(mine), stride, ctypes.byref(m), ctypes.byref(x)) == 0
                maxima.append((m.value, x.value))
            mm, mx = max(m for m, _ in maxima), max(x for _, x in maxima)
            for c in ctxs:
                c.upload_finish(mm, mx)
                c.compute_accel()
                out.append((c.forces(G), c.effective_tuning(), c.close_set_mode()[0]))
        finally:
            for c in reversed(ctxs):                        # rank 0 owns the buffers: it goes last
                c.close()
        return maxima, out

    ref_max, ref_out = sharded(_min_stride(dim))
    full = oracle.brute_force_seq(b)
    S = oracle.force_magnitude_sums(b)
    L = -(-n // shards)
    for r, (f, _, _) in enumerate(ref_out):
        assert_force_parity(f, full[r * L:r * L + f.shape[0]], S[r * L:r * L + f.shape[0]], f"sharded upload, rank {r}", n_sources=n)
    for stride in _strides(dim):
        got_max, got_out = sharded(stride)
        assert got_max == ref_max, (stride, got_max, ref_max)       # a misread column shows up in max |mass| / |coordinate|
        for r in range(shards):
            assert _same_bits(got_out[r][0], ref_out[r][0]), f"upload_shard stride={stride}: rank {r} forces differ"
            assert got_out[r][1:] == ref_out[r][1:]

    # download: only this shard's rows change, and only their first 2D columns
    dt, Gs = 2.0, oracle.G * 1e24
    for r in range(shards):
        with nbx.Context(n, dim, n_shards=shards, shard=r) as c:
            c.upload(b)
            c.compute_accel()
            c.kick_drift(dt, Gs)
            ref = b.copy()
            c.download(ref)
            lo, hi = r * c.shard_len, r * c.shard_len + c.count
            assert not _same_bits(ref[lo:hi, :2 * dim], b[lo:hi, :2 * dim]), "the kick/drift must have moved the state"
            for stride in _strides(dim):
                dst = _sentinel_array((n, stride // 8))
                keep = dst.copy()
                assert lib.nbx_ctx_download_bodies(c.h, _ptr(dst), stride) == 0
                assert _same_bits(dst[lo:hi, :2 * dim], ref[lo:hi, :2 * dim]), f"rank {r} stride={stride}: downloaded state differs"
                assert _same_bits(dst[lo:hi, 2 * dim:], keep[lo:hi, 2 * dim:]), f"rank {r} stride={stride}: mass / extra columns written"
                assert _same_bits(dst[:lo], keep[:lo]) and _same_bits(dst[hi:], keep[hi:]), f"rank {r} stride={stride}: other rows written"


def test_node_at_wide_strides(nbx, oracle):
    """nbx_node_upload_bodies / forces / step / nbx_node_download_bodies on three virtual ranks."""
    lib = _lib(nbx)
    n, dim, steps, dt = 4000, 3, 3, 2.0
    G = oracle.G * 1e24
    b = _inputs(oracle, 307, n, dim)

    def run(stride):
        src = b if stride == _min_stride(dim) else _wide(b, stride)
        keep = src.copy()
        with nbx.Node(n, dim, [0, 0, 0]) as node:
            assert lib.nbx_node_upload_bodies(node.h, _ptr(src), stride) == 0
            f = node.forces(oracle.G)
            node.step(dt, steps, G)
            node.synchronize()
            dst = keep.copy()
            assert lib.nbx_node_download_bodies(node.h, _ptr(dst), stride) == 0
        assert _same_bits(src, keep)
        assert _same_bits(dst[:, 2 * dim:], keep[:, 2 * dim:]), f"stride={stride}: mass / extra columns written"
        return f, dst[:, :2 * dim]

    ref_f, ref_state = run(_min_stride(dim))
    assert_force_parity(ref_f, oracle.brute_force_seq(b), oracle.force_magnitude_sums(b), "node, three virtual ranks")
    assert not _same_bits(ref_state, b[:, :2 * dim])
    for stride in _strides(dim):
        f, state = run(stride)
        assert _same_bits(f, ref_f) and _same_bits(state, ref_state), f"node stride={stride}"


@pytest.mark.parametrize("dim", (3, 2))
def test_leaf_pairs_at_wide_strides(nbx, oracle, dim):
    """nbx_leaf_pair_forces through both planners; one plan fed min -> 256 B -> min + 8 -> min (the second call regrows the plan's
    staged bodies); nbx_leaf_plan_get_forces after a wide call, which reads the masses at the caller's stride."""
    lib = _lib(nbx)
    n = 3000
    b = _inputs(oracle, 308, n, dim)
    leaves = _csr(nbx.leaves.uniform_grid_leaves(b, dim, 3 if dim == 3 else 5))
    nl = leaves[0].size - 1
    G = oracle.G
    for law in (nbx.LAW_BRUTE, nbx.LAW_FMM_P2P):
        for which in ("host", "device"):
            with planner(which):
                ref = nbx.leaf_pair_forces_hip(b, *leaves, law=law, G=G)
                for stride in _strides(dim):
                    w = _wide(b, stride)
                    keep = w.copy()
                    out = np.empty((n, dim))
                    assert lib.nbx_leaf_pair_forces(_ptr(w), n, dim, stride, _ptr(leaves[0]), _ptr(leaves[1]), nl, _ptr(leaves[2]),
                                                    _ptr(leaves[3]), law, G, 0, _ptr(out), None) == 0
                    assert _same_bits(out, ref), f"one-shot law={law} planner={which} stride={stride}"
                    assert _same_bits(w, keep)
                with nbx.LeafPlan(n, dim, *leaves) as plan:
                    m = _min_stride(dim)
                    for k, stride in enumerate((m, 256, m + 8, m)):
                        w = b if stride == m else _wide(b, stride)
                        out = _sentinel_array((n, dim))
                        assert lib.nbx_leaf_plan_forces(plan.h, _ptr(w), stride, law, G, _ptr(out), None) == 0
                        assert _same_bits(out, ref), f"plan call {k} law={law} planner={which} stride={stride}"
                        assert _same_bits(plan.get_forces(), ref), f"get_forces after call {k} (stride {stride})"


# ---- rejected strides ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", (3, 2))
def test_rejected_strides_change_nothing(nbx, oracle, dim):
    """A stride below sizeof(Body<dim>), not a multiple of 8, or 0 is NBX_ERR_INVALID from every entry point that takes one; the caller's
    buffers keep their bits and the context, node or plan answers afterwards as before."""
    lib = _lib(nbx)
    n, G = 600, oracle.G
    b = _inputs(oracle, 309, n, dim)
    wide = _wide(b, 256)                                     # room behind every record for what a wrong stride would reach
    bad = _bad_strides(dim)

    def untouched(a, keep, what):
        assert _same_bits(a, keep), f"{what}: a refused call wrote the caller's array"

    for s in bad:
        out = _sentinel_array((n, dim))
        keep = out.copy()
        info = nbx.EvalInfo()
        assert lib.nbx_brute_force_forces(_ptr(wide), n, dim, s, G, 0, _ptr(out), None) == NBX_ERR_INVALID, s
        untouched(out, keep, f"nbx_brute_force_forces stride={s}")
        assert lib.nbx_brute_force_forces_ex(_ptr(wide), n, dim, s, G, 0, 0.0, _ptr(out), ctypes.byref(info)) == NBX_ERR_INVALID, s
        untouched(out, keep, f"nbx_brute_force_forces_ex stride={s}")
        arr = wide.copy()
        assert lib.nbx_leapfrog(_ptr(arr), n, dim, s, G, 1.0, 2, 0, None) == NBX_ERR_INVALID, s
        untouched(arr, wide, f"nbx_leapfrog stride={s}")

    shards = 3
    for r in range(shards):
        with nbx.Context(n, dim, n_shards=shards, shard=r) as c:
            c.upload(b)
            c.compute_accel()
            before = c.forces(G)
            lo = r * c.shard_len
            mine = np.ascontiguousarray(wide[lo:lo + c.count])
            for s in bad:
                assert lib.nbx_ctx_upload_bodies(c.h, _ptr(wide), s) == NBX_ERR_INVALID, s
                m, x = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
                assert lib.nbx_ctx_upload_shard(c.h, _ptr(mine), s, ctypes.byref(m), ctypes.byref(x)) == NBX_ERR_INVALID, s
                assert m.value == -1.0 and x.value == -1.0
                dst = _sentinel_array((n, 32))
                keep = dst.copy()
                assert lib.nbx_ctx_download_bodies(c.h, _ptr(dst), s) == NBX_ERR_INVALID, s
                untouched(dst, keep, f"nbx_ctx_download_bodies stride={s}")
            c.compute_accel()                               # the context still holds what the last good upload left
            assert _same_bits(c.forces(G), before), f"rank {r}: forces changed after refused uploads"
            c.upload(b)
            c.compute_accel()
            assert _same_bits(c.forces(G), before)

    with nbx.Node(n, dim, [0, 0, 0]) as node:
        node.upload(b)
        before = node.forces(G)
        for s in bad:
            assert lib.nbx_node_upload_bodies(node.h, _ptr(wide), s) == NBX_ERR_INVALID, s
            dst = _sentinel_array((n, 32))
            keep = dst.copy()
            assert lib.nbx_node_download_bodies(node.h, _ptr(dst), s) == NBX_ERR_INVALID, s
            untouched(dst, keep, f"nbx_node_download_bodies stride={s}")
        assert _same_bits(node.forces(G), before)

    leaves = _csr(nbx.leaves.uniform_grid_leaves(b, dim, 2))
    nl = leaves[0].size - 1
    law = nbx.LAW_FMM_P2P
    ref = nbx.leaf_pair_forces_hip(b, *leaves, law=law, G=G)
    for s in bad:
        out = _sentinel_array((n, dim))
        keep = out.copy()
        assert lib.nbx_leaf_pair_forces(_ptr(wide), n, dim, s, _ptr(leaves[0]), _ptr(leaves[1]), nl, _ptr(leaves[2]), _ptr(leaves[3]),
                                        law, G, 0, _ptr(out), None) == NBX_ERR_INVALID, s
        untouched(out, keep, f"nbx_leaf_pair_forces stride={s}")
    with nbx.LeafPlan(n, dim, *leaves) as plan:
        assert _same_bits(plan.forces(b, law, G), ref)
        for s in bad:
            out = _sentinel_array((n, dim))
            keep = out.copy()
            assert lib.nbx_leaf_plan_forces(plan.h, _ptr(wide), s, law, G, _ptr(out), None) == NBX_ERR_INVALID, s
            untouched(out, keep, f"nbx_leaf_plan_forces stride={s}")
        assert _same_bits(plan.get_forces(), ref), "the plan's last evaluation survives refused calls"
        assert _same_bits(plan.forces(b, law, G), ref)


# ---- degenerate partitions ----------------------------------------------------------------------------------------------

def _planted(oracle, seed, n, dim, shards):
    """Oracle input with, for N >= 2, a pair at r^2 < 1e-10 (skipped) and, where a second disjoint boundary pair exists, one at
    1e-10 <= r^2 < 1e-6 (counted), each straddling a shard boundary (the values of cross_shard_case.py)."""
    b = oracle.generate(seed, n, dim)
    L = csc.shard_len(n, shards) if n else 0
    pairs = []
    for k in range(1, shards):
        e = k * L
        if e >= n or e < 1:
            break
        pairs.append((e - 1, e))
        if e >= 2 and e + 1 < n:
            pairs.append((e - 2, e + 1))
    special = []
    if pairs:
        plan = [(pairs[0], 3.0, 3.0 + 4.8e-7, 1)]                         # r^2 = 2.3e-13
        rest = [p for p in pairs[1:] if not set(p) & set(pairs[0])]
        if rest:
            plan.append((rest[0], 100.0, 100.0 + 1.6e-5, 2))             # r^2 = 2.6e-10
        for (i, j), a, c, k in plan:
            far = [2.0e6 + 1.0e5 * k, 3.0e6 + 1.0e5 * k, 4.0e6][:dim]
            b[i, :dim] = far
            b[j, :dim] = far
            b[i, k % dim] = a
            b[j, k % dim] = c
            special += [i, j]
    return oracle.round_inputs_to_f32(b), special


def _reference_rows(oracle, b, special, shards):
    n = b.shape[0]
    if n <= 10000:
        rows = np.arange(n)
        return rows, oracle.brute_force_seq(b), oracle.force_magnitude_sums(b)
    L = csc.shard_len(n, shards)
    edges = [e + d for e in range(0, n, L) for d in (-1, 0, 1)] + [n - 1]
    rows = np.unique(np.r_[np.arange(0, n, 97), special, edges].astype(np.int64))
    rows = rows[(rows >= 0) & (rows < n)]
    return rows, oracle.force_rows_omp_2(b, rows), oracle.force_magnitude_sums(b, rows)


PARTITIONS = [(0, 1, 3), (0, 3, 2), (1, 2, 3), (2, 3, 2), (5, 8, 3), (8, 8, 2), (9, 8, 3), (7, 3, 2), (32768, 8, 3), (32769, 8, 2)]


@pytest.mark.parametrize("n,shards,dim", PARTITIONS)
def test_degenerate_partitions(nbx, oracle, n, shards, dim):
    """Every shard of N bodies on `shards` contexts, empty and one-body shards included: ALL and LOCAL + REMOTE passes against the
    oracle, every target refined against the strict bounds, the exports of an empty shard, and the shards' energies against the
    oracle's.  Twice: with planted close pairs straddling a boundary, and without.  A shard of a few bodies that holds a planted pair
    has more than 1/8 of its targets owning a pair closer than 1e-3, so the library runs the guarded kernel there, where the mixed mode
    does not apply (include/nbody_hip.h, nbx_ctx_set_tuning / nbx_ctx_set_refine); the input without planted pairs refines every shard."""
    G = oracle.G
    L = -(-n // shards)
    for planted in (True, False):
        if planted:
            b, special = _planted(oracle, 400 + n, n, dim, shards)
        else:
            b, special = _inputs(oracle, 450 + n, n, dim), []
        rows, ref, S = _reference_rows(oracle, b, special, shards)
        tot = np.zeros(2)
        counts = []
        for r in range(shards):
            with nbx.Context(n, dim, n_shards=shards, shard=r) as c:
                cnt = min(L, max(0, n - r * L))
                lo = r * L
                assert c.shard_len == L and c.shard_pad == max(4096, -(-L // 4096) * 4096) and c.count == cnt, (c.shard_len, c.shard_pad, c.count)
                counts.append(cnt)
                what = f"N={n} shards={shards} D={dim} rank {r} ({cnt} bodies{', planted pairs' if planted else ''})"
                mine = (rows >= lo) & (rows < lo + cnt)
                loc, ref_s, S_s = rows[mine] - lo, ref[mine], S[mine]
                c.upload(b)
                guarded = c.close_set_mode()[0] == "guarded_kernel"
                assert not guarded or (planted and cnt), f"{what}: only a shard holding a planted pair may leave the fast path"
                c.compute_accel()
                f_all = c.forces(G)
                assert f_all.shape == (cnt, dim), what
                if cnt:
                    assert_force_parity(f_all[loc], ref_s, S_s, what + ", ALL", n_sources=n)
                if n <= 10000:     # the device's accuracy metric reads `count` reference rows (utils.h:170-219 on the device)
                    ref_shard = np.ascontiguousarray(ref[lo:lo + cnt])
                    assert c.accuracy(ref_shard, G) == oracle.compute_accuracy(f_all, ref_shard), what
                c.compute_accel(nbx.SRC_LOCAL)
                c.compute_accel(nbx.SRC_REMOTE)
                f_lr = c.forces(G)
                assert f_lr.shape == (cnt, dim), what
                if cnt:
                    assert_force_parity(f_lr[loc], ref_s, S_s, what + ", LOCAL + REMOTE", n_sources=n)
                c.set_refine(1e-7, 1e6)                         # every target is a suspect ...
                listed = cnt if n >= 2 else 0                   # ... but a lone body, whose sum has no term: its zero is exact
                for passes in ((nbx.SRC_ALL,), (nbx.SRC_LOCAL, nbx.SRC_REMOTE)):
                    for p in passes:
                        c.compute_accel(p)
                    if guarded:
                        with pytest.raises(nbx.NbxError) as e:
                            c.refine_stats()
                        assert e.value.status == NBX_ERR_STATE
                        continue
                    assert c.refine_stats() == (listed, listed), (what, passes, c.refine_stats())
                    f_strict = c.forces(G)
                    assert f_strict.shape == (cnt, dim)
                    if cnt:
                        _assert_strict(f_strict[loc], ref_s, S_s, what + f", every target refined, passes {passes}")
                if not guarded:
                    assert c.aux().shape == (cnt,)
                ke, pe = c.energy(G)
                tot += (ke, pe)
                if cnt == 0:
                    assert c.forces(G).shape == (0, dim) and c.accel().shape == (dim, 0) and c.refine_stats() == (0, 0)
                    assert (ke, pe) == (0.0, 0.0), what
                    assert c.accuracy(np.zeros((0, dim)), G) == 0.0
                    c.kick_drift(1.0, G)
                    dst = _sentinel_array((n, 2 * dim + 1))
                    keep = dst.copy()
                    c.download(dst)
                    assert _same_bits(dst, keep), f"{what}: an empty shard's download wrote the array"
        assert sum(counts) == n
        ke_ref, pe_ref = oracle.energy(b)
        assert abs(tot[0] - ke_ref) <= 1e-13 * ke_ref and abs(tot[1] - pe_ref) <= 2e-6 * pe_ref, (n, shards, planted, tot, ke_ref, pe_ref)


@pytest.mark.parametrize("n", (1, 5, 9, 8195))
def test_node_with_empty_and_short_ranks(nbx, oracle, n):
    """Eight virtual ranks with empty ranks (N = 1, 5), one-body ranks (N = 9: shard_len 2, the last rank holds one) and a short last
    rank (N = 8195: shard_len 1025): forces with planted cross-boundary pairs against the oracle, then four coupled steps against the
    oracle's trajectory (the protocol of test_gpu_node.py::test_virtual_ranks_forces_and_steps)."""
    dim, ranks = 3, 8
    bp, _ = _planted(oracle, 500 + n, n, dim, ranks)
    with nbx.Node(n, dim, [0] * ranks) as node:
        node.upload(bp)
        assert node.verify_exchange() == 0
        f = node.forces(oracle.G)
    assert f.shape == (n, dim)
    assert_force_parity(f, oracle.brute_force_seq(bp), oracle.force_magnitude_sums(bp), f"node N={n}, {ranks} virtual ranks")

    b = _inputs(oracle, 600 + n, n, dim)
    gscale = 1e24 if n > 1000 else 1e30                      # a few bodies need a stronger coupling to move measurably
    G = oracle.G * gscale
    steps, dt = 4, 2.0
    with nbx.Node(n, dim, [0] * ranks) as node:
        node.upload(b)
        node.step(dt, steps, G)
        node.synchronize()
        got = b.copy()
        node.download(got)
        ke, pe = node.energy(G)
    cur = b.copy()
    for _ in range(steps):
        ff = oracle.brute_force_seq(oracle.round_inputs_to_f32(cur)) * gscale
        oracle.update_body_velocities(cur, np.ascontiguousarray(ff), dt)
        oracle.update_body_positions(cur, dt)
    d = dim
    moved = np.abs(cur[:, d:2 * d] - b[:, d:2 * d]).max()
    if n == 1:
        assert moved == 0.0 and _same_bits(got, cur), "a lone body drifts with its velocity"
    else:
        assert moved > 1e-6, "coupling too weak to move the bodies measurably"
        assert np.allclose(got[:, d:2 * d], cur[:, d:2 * d], rtol=0, atol=3e-5 * moved)
        assert np.allclose(got[:, :d], cur[:, :d], rtol=1e-9, atol=3e-5 * moved * dt * steps)
    assert _same_bits(got[:, 2 * d:], b[:, 2 * d:])
    r32 = oracle.round_inputs_to_f32(got)
    r32[:, d:2 * d] = got[:, d:2 * d]
    ke_ref, pe_ref = oracle.energy(r32)
    assert abs(ke - ke_ref) <= 1e-12 * ke_ref and abs(pe - pe_ref * gscale) <= 3e-6 * pe_ref * gscale


# ---- raw accelerations --------------------------------------------------------------------------------------------------

MODES = ("plain", "mixed", "softened", "newton")
EPS = 40.0


@pytest.mark.parametrize("dim", (3, 2))
def test_raw_accelerations(nbx, oracle, dim):
    """nbx_ctx_get_accel is float[dim][count]: for every variant, plain and mixed mode, the softened and the Newtonian law, one shard and
    three (the last one short), forces[l, k] = -(G' m_l) accel[k, l] to the fp32 rounding of the sum (G' = -G for the attractive law),
    and -(G' m) accel passes the force parity against the oracle.  The raw call writes count x dim values and nothing behind them."""
    lib = _lib(nbx)
    n, G = 2500, oracle.G
    u = 2.0 ** -24
    b = _inputs(oracle, 310, n, dim)
    m = b[:, 2 * dim]
    refs = {"plain": (oracle.brute_force_seq(b), oracle.force_magnitude_sums(b)),
            "softened": oracle.force_rows_softened(b, EPS), "newton": oracle.force_rows_softened(b, EPS, newton=True)}
    refs["mixed"] = refs["plain"]
    for shards in (1, 3):
        for r in range(shards):
            with nbx.Context(n, dim, n_shards=shards, shard=r) as c:
                c.upload(b)
                cnt, lo = c.count, r * c.shard_len
                for v, name in enumerate(nbx.variants()):
                    for mode in MODES:
                        what = f"D={dim} rank {r}/{shards} {name} {mode}"
                        c.set_tuning(0, v)
                        c.set_refine(1e-5 if mode == "mixed" else 0.0)
                        c.set_softening(EPS if mode in ("softened", "newton") else 0.0)
                        c.set_law(nbx.FORCE_LAW_NEWTON if mode == "newton" else nbx.FORCE_LAW_REFERENCE)
                        c.compute_accel()
                        f = c.forces(G)
                        raw = _sentinel_array(dim * c.shard_len + 8, np.float32)
                        keep = raw.copy()
                        assert lib.nbx_ctx_get_accel(c.h, _ptr(raw)) == 0
                        assert _same_bits(raw[dim * cnt:], keep[dim * cnt:]), f"{what}: get_accel wrote past dim x count"
                        a = c.accel()
                        assert a.shape == (dim, cnt) and _same_bits(a.reshape(-1), raw[:dim * cnt]), what
                        Gp = -G if mode == "newton" else G
                        pred = -(Gp * m[lo:lo + cnt])[:, None] * a.T.astype(np.float64)
                        assert (np.abs(f - pred) <= 1.0001 * u * np.abs(f)).all(), \
                            f"{what}: forces and accelerations disagree by {np.max(np.abs(f - pred) / np.maximum(np.abs(f), 1e-300)):.3e}"
                        ref, S = refs[mode]
                        assert_force_parity(pred, ref[lo:lo + cnt], S[lo:lo + cnt], what, n_sources=n)
