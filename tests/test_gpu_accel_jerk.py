"""GPU: accelerations and jerks of a list of targets (nbx_ctx_compute_accel_jerk_active / nbx_ctx_get_accel_jerk_active,
csrc/active_jerk_kernel.hip).  The shapes are tests/test_gpu_active_forces.py's: N at the edges of a source tile (256) and of the pad
quantum (4,096); lists at the edges of a wave (64), of a list block of either build (256 and 1,024), empty, and as long as N;
shuffled, with repeated indices; both builds through NBODY_HIP_ACTIVE_LONG_LIST, both laws, D = 2 and 3.  Velocities are the
generator's, rounded to fp32; bodies 10 and 11 coincide and move differently.

Accelerations: scaled by the target's mass they are the forces of oracle.force_rows_softened, under assert_force_parity.
Jerks: |dJ_r| <= 1e-5 S_j against hermite.accel_jerk_rows (fp64), S_j = |G| sum_j m_j w |dv| (1 + p r^2 / rho^2) -- the constant of
(T1) on the bound of each pair term's magnitude: the tile summation and the pair arithmetic are those of the force.  The worst
ratio |dJ_r| / (1e-5 S_j) is printed per case."""
import ctypes

import numpy as np
import pytest

from oracle_lib import TOL_BACKWARD, assert_force_parity

pytestmark = pytest.mark.gpu

LONG_BLOCK = 1024                                                # targets per workgroup of the long-list build (nbx_internal.h: kJerkLongBlock)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, LONG_BLOCK - 1, LONG_BLOCK, LONG_BLOCK + 1)
SIZES = (1, 2, 255, 256, 257, 4096, 4097)
BUILDS = {"short": str(1 << 31), "long": "1"}
EPS = {False: 50.0, True: 2.0e4}                                 # tests/test_gpu_softening.py's softening lengths for the two laws
JERK_TOL = 1.0e-5
assert JERK_TOL == TOL_BACKWARD

_cache = {}


def system(nbx, oracle, dim, n, newton):
    """(bodies, forces, force magnitude sums, jerks, S_j) of all rows, computed once per shape and left unchanged"""
    key = (dim, n, newton)
    if key not in _cache:
        b = oracle.generate(300 + dim, n, dim)
        if n > 11:
            b[11, :dim] = b[10, :dim]                            # a coincident pair: zero force between them, the jerk term m dv / eps^p
            assert not np.array_equal(b[11, dim:2 * dim], b[10, dim:2 * dim])
        b = oracle.round_inputs_to_f32(b)
        b[:, dim:2 * dim] = b[:, dim:2 * dim].astype(np.float32)  # the velocities too: the device's sources are the checker's
        ref, S = oracle.force_rows_softened(b, EPS[newton], newton=newton)
        jerk, S_j = np.zeros((n, dim)), np.zeros(n)
        for lo in range(0, n, 512):                              # in blocks of rows: the pair arrays stay small
            rows = np.arange(lo, min(lo + 512, n))
            _, jerk[rows], _, S_j[rows] = nbx.hermite.accel_jerk_rows(b, rows, oracle.G, EPS[newton], "newton" if newton else "soft")
        for a in (b, ref, S, jerk, S_j):
            a.setflags(write=False)
        _cache[key] = (b, ref, S, jerk, S_j)
    return _cache[key]


def context(nbx, monkeypatch, b, dim, newton, build):
    monkeypatch.setenv("NBODY_HIP_ACTIVE_LONG_LIST", BUILDS[build])
    c = nbx.Context(b.shape[0], dim)
    c.upload(b)
    c.set_softening(EPS[newton])
    if newton:
        c.set_law(nbx.FORCE_LAW_NEWTON)
    return c


def jerk_ratio(j, jerk_ref, S_j):
    """largest |dJ_r| / (JERK_TOL S_j) over the rows; a row whose S_j is 0 (no other body moves against it) must be exact"""
    dJ = np.sqrt(((j - jerk_ref) ** 2).sum(axis=1))
    assert (dJ[S_j == 0] == 0).all()
    live = S_j > 0
    return float((dJ[live] / (JERK_TOL * S_j[live])).max()) if live.any() else 0.0


@pytest.mark.parametrize("build", tuple(BUILDS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("newton", (False, True))
@pytest.mark.parametrize("dim", (3, 2))
def test_listed_accelerations_and_jerks_match_the_checker(nbx, oracle, monkeypatch, dim, newton, n, build):
    b, ref, S, jerk_ref, S_j = system(nbx, oracle, dim, n, newton)
    rng = np.random.default_rng(7 * n + dim)
    worst = 0.0
    with context(nbx, monkeypatch, b, dim, newton, build) as c:
        for length in LENGTHS + (n,):
            targets = rng.permutation(n) if length == n else rng.integers(0, n, size=length)     # shuffled; repeats unless a permutation
            c.compute_accel_jerk_active(targets)
            a, j = c.accel_jerk_active(oracle.G)
            assert a.shape == j.shape == (length, dim)
            if length:
                what = f"D={dim} newton={newton} N={n} list of {length}, {build} build"
                assert_force_parity(a * b[targets, -1][:, None], ref[targets], S[targets], what, n_sources=n)
                assert np.isfinite(j).all(), what
                ratio = jerk_ratio(j, jerk_ref[targets], S_j[targets])
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{what}: |dJ| = {ratio:.3f} x 1e-5 S_j"
            first = {}
            for r, t in enumerate(targets):                      # a repeated index is evaluated by itself, to the same bits
                at = first.setdefault(int(t), r)
                assert np.array_equal(a[r], a[at]) and np.array_equal(j[r], j[at])
    print(f"D={dim} newton={newton} N={n} {build}: worst |dJ_r| / (1e-5 S_j) = {worst:.3f}")


@pytest.mark.parametrize("dim", (3, 2))
def test_the_two_builds_agree_and_each_repeats_its_bits(nbx, oracle, monkeypatch, dim):
    n = 4097
    b, ref, S, jerk_ref, S_j = system(nbx, oracle, dim, n, True)
    targets = np.random.default_rng(5).integers(0, n, size=LONG_BLOCK + 1)
    got = {}
    for build in BUILDS:
        with context(nbx, monkeypatch, b, dim, True, build) as c:
            c.compute_accel_jerk_active(targets)
            got[build] = c.accel_jerk_active(oracle.G)
            c.compute_accel_jerk_active(targets[:65])            # another list in between
            c.compute_accel_jerk_active(targets)
            again = c.accel_jerk_active(oracle.G)
            assert np.array_equal(got[build][0], again[0]) and np.array_equal(got[build][1], again[1])
    m = b[targets, -1][:, None]
    assert_force_parity(got["short"][0] * m, got["long"][0] * m, S[targets], "short build against long build", n_sources=n)
    assert jerk_ratio(got["short"][1], got["long"][1], S_j[targets]) <= 1.0


@pytest.mark.parametrize("build", tuple(BUILDS))
def test_the_call_is_an_observer(nbx, oracle, monkeypatch, build):
    dim, n = 3, 4097
    b, ref, S, jerk_ref, S_j = system(nbx, oracle, dim, n, False)
    with context(nbx, monkeypatch, b, dim, False, build) as c:
        c.compute_accel()
        f0 = c.forces(oracle.G)
        c.compute_accel_jerk_active(np.arange(n)[::-1])
        a, j = c.accel_jerk_active(oracle.G)
        assert np.array_equal(c.forces(oracle.G), f0)            # the context's accelerations stand, bit for bit
        assert_force_parity((a * b[::-1, -1][:, None])[::-1], f0, S, "all bodies through the list against nbx_ctx_compute_accel", n_sources=n)
        got = b.copy()
        c.kick_drift2(0.0, 0.0)                                   # still allowed: have_accel was not touched
        c.download(got)
        assert np.array_equal(got, b)
        only_a, only_j = np.full((n, dim), 7.0), np.full((n, dim), 7.0)
        lib = nbx.load_library()
        assert lib.nbx_ctx_get_accel_jerk_active(c.h, oracle.G, only_a.ctypes.data, None) == 0      # either output may be null
        assert lib.nbx_ctx_get_accel_jerk_active(c.h, oracle.G, None, only_j.ctypes.data) == 0
        assert np.array_equal(only_a, a) and np.array_equal(only_j, j)


def test_a_massless_tracer_keeps_its_row(nbx, oracle, monkeypatch):
    dim, n = 3, 257
    b, ref, S, jerk_ref, S_j = system(nbx, oracle, dim, n, True)
    t = b.copy()
    t[5, -1] = 0.0
    a_ref, j_ref, S_a, S_jt = nbx.hermite.accel_jerk_rows(t, np.array([5, 6]), oracle.G, EPS[True], "newton")
    with context(nbx, monkeypatch, t, dim, True, "short") as c:
        c.compute_accel_jerk_active([5, 6])
        a, j = c.accel_jerk_active(oracle.G)
    assert np.isfinite(a).all() and np.isfinite(j).all() and np.abs(a[0]).max() > 0
    assert (np.sqrt(((a - a_ref) ** 2).sum(axis=1)) <= 1.0e-5 * S_a).all()
    assert jerk_ratio(j, j_ref, S_jt) <= 1.0


def test_refusals(nbx, oracle, monkeypatch):
    dim, n = 3, 257
    b, *_ = system(nbx, oracle, dim, n, False)
    lib = nbx.load_library()
    NBX_ERR_INVALID, NBX_ERR_STATE = 1, 5
    t = np.arange(4, dtype=np.uint32)
    out_a, out_j = np.full((4, dim), 7.0), np.full((4, dim), 7.0)
    get = lambda c: lib.nbx_ctx_get_accel_jerk_active(c.h, ctypes.c_double(oracle.G), out_a.ctypes.data, out_j.ctypes.data)
    with nbx.Context(n, dim) as c:
        assert lib.nbx_ctx_compute_accel_jerk_active(c.h, t.ctypes.data, 4) == NBX_ERR_STATE     # nothing uploaded
        c.upload(b)
        assert lib.nbx_ctx_compute_accel_jerk_active(c.h, t.ctypes.data, 4) == NBX_ERR_STATE     # softening 0
        c.set_softening(EPS[False])
        assert get(c) == NBX_ERR_STATE                                                            # nothing computed yet
        assert lib.nbx_ctx_compute_accel_jerk_active(c.h, None, 4) == NBX_ERR_INVALID
        bad = np.array([0, n, 1], dtype=np.uint32)
        assert lib.nbx_ctx_compute_accel_jerk_active(c.h, bad.ctypes.data, 3) == NBX_ERR_INVALID and "n_total" in lib.nbx_last_error_detail().decode()
        assert get(c) == NBX_ERR_STATE and (out_a == 7.0).all() and (out_j == 7.0).all()
        c.compute_accel_jerk_active(t)
        assert get(c) == 0
        c.compute_accel_active(t)                                                                  # the twin takes the list over
        assert get(c) == NBX_ERR_STATE
        c.compute_accel_jerk_active([])                                                            # an empty list is legal
        a, j = c.accel_jerk_active(oracle.G)
        assert a.shape == j.shape == (0, dim)
        c.compute_accel_jerk_active(t)
        c.upload(b)                                                                                # an upload ends the sums' validity
        assert get(c) == NBX_ERR_STATE
        heavy = b.copy()
        heavy[:, -1] *= 1.0e9                                                                      # masses up to 1e17 over eps^4 = 1e-24:
        c.upload(heavy)
        c.set_softening(1.0e-6)                                                                    # m / eps^4 out of fp32 range, nbx_ctx_compute_accel's rule
        assert lib.nbx_ctx_compute_accel_jerk_active(c.h, t.ctypes.data, 4) == lib.nbx_ctx_compute_accel(c.h, 0) == NBX_ERR_INVALID
    with nbx.Context(n, dim, n_shards=2, shard=0) as c:
        c.upload(b)
        c.set_softening(EPS[False])
        assert lib.nbx_ctx_compute_accel_jerk_active(c.h, t.ctypes.data, 4) == NBX_ERR_STATE
