"""GPU: forces on a list of targets (nbx_ctx_compute_accel_active / nbx_ctx_get_forces_active, csrc/active_kernel.hip) against the
oracle's fp64 restatement of the softened laws, oracle.force_rows_softened(rows = the list), under the tolerances of every force test
(assert_force_parity).  Every shape runs under BOTH builds of the kernel -- one target per lane and eight -- through
NBODY_HIP_ACTIVE_LONG_LIST, which a context reads when it is created: 1 sends every list to the long-list build, 2^31 every list to
the short one.  The shapes: N at the edges of a source tile (256) and of the pad quantum (4,096), and 6,000; lists at the edges of a
wave (64), of a list block of either build (256 and 2,048), empty, and as long as N; shuffled, with repeated indices."""
import ctypes

import numpy as np
import pytest

from oracle_lib import assert_force_parity

pytestmark = pytest.mark.gpu

LONG_BLOCK = 2048                                                # targets per workgroup of the long-list build (nbx_internal.h: kActiveLongBlock)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, LONG_BLOCK - 1, LONG_BLOCK, LONG_BLOCK + 1)
SIZES = (1, 2, 255, 256, 257, 4096, 4097, 6000)
BUILDS = {"short": str(1 << 31), "long": "1"}
EPS = {False: 50.0, True: 2.0e4}                                 # tests/test_gpu_softening.py's softening lengths for the two laws

_cache = {}


def system(oracle, dim, n, newton):
    """(bodies, forces of all rows, magnitude sums of all rows), computed once per shape and left unchanged"""
    key = (dim, n, newton)
    if key not in _cache:
        b = oracle.generate(300 + dim, n, dim)
        if n > 11:
            b[11, :dim] = b[10, :dim]                            # a coincident pair: zero force between them, finite weights
        b = oracle.round_inputs_to_f32(b)
        ref, S = oracle.force_rows_softened(b, EPS[newton], newton=newton)
        for a in (b, ref, S):
            a.setflags(write=False)
        _cache[key] = (b, ref, S)
    return _cache[key]


def context(nbx, monkeypatch, b, dim, newton, build):
    monkeypatch.setenv("NBODY_HIP_ACTIVE_LONG_LIST", BUILDS[build])
    c = nbx.Context(b.shape[0], dim)
    c.upload(b)
    c.set_softening(EPS[newton])
    if newton:
        c.set_law(nbx.FORCE_LAW_NEWTON)
    return c


@pytest.mark.parametrize("build", tuple(BUILDS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("newton", (False, True))
@pytest.mark.parametrize("dim", (3, 2))
def test_listed_forces_match_the_checker(nbx, oracle, monkeypatch, dim, newton, n, build):
    b, ref, S = system(oracle, dim, n, newton)
    rng = np.random.default_rng(7 * n + dim)
    with context(nbx, monkeypatch, b, dim, newton, build) as c:
        for length in LENGTHS + (n,):
            targets = rng.permutation(n) if length == n else rng.integers(0, n, size=length)     # shuffled; repeats unless a permutation
            c.compute_accel_active(targets)
            f = c.forces_active(oracle.G)
            assert f.shape == (length, dim)
            if length:
                assert_force_parity(f, ref[targets], S[targets], f"D={dim} newton={newton} N={n} list of {length}, {build} build", n_sources=n)
            first = {}
            for r, t in enumerate(targets):                      # a repeated index is evaluated by itself, to the same bits
                assert np.array_equal(f[r], f[first.setdefault(int(t), r)])


@pytest.mark.parametrize("dim", (3, 2))
def test_the_two_builds_agree_and_each_repeats_its_bits(nbx, oracle, monkeypatch, dim):
    n = 4097
    b, ref, S = system(oracle, dim, n, True)
    targets = np.random.default_rng(5).integers(0, n, size=LONG_BLOCK + 1)
    got = {}
    for build in BUILDS:
        with context(nbx, monkeypatch, b, dim, True, build) as c:
            c.compute_accel_active(targets)
            got[build] = c.forces_active(oracle.G)
            c.compute_accel_active(targets[:65])                 # another list in between
            c.compute_accel_active(targets)
            assert np.array_equal(got[build], c.forces_active(oracle.G))
    assert_force_parity(got["short"], got["long"], S[targets], "short build against long build", n_sources=n)


@pytest.mark.parametrize("build", tuple(BUILDS))
def test_the_call_is_an_observer(nbx, oracle, monkeypatch, build):
    dim, n = 3, 4097
    b, ref, S = system(oracle, dim, n, False)
    with context(nbx, monkeypatch, b, dim, False, build) as c:
        c.compute_accel()
        f0 = c.forces(oracle.G)
        c.compute_accel_active(np.arange(n)[::-1])
        fa = c.forces_active(oracle.G)
        assert np.array_equal(c.forces(oracle.G), f0)            # the context's accelerations stand, bit for bit
        assert_force_parity(fa[::-1], f0, S, "all bodies through the list against nbx_ctx_compute_accel", n_sources=n)
        got = b.copy()
        c.kick_drift2(0.0, 0.0)                                   # still allowed: have_accel was not touched
        c.download(got)
        assert np.array_equal(got, b)


def test_refusals(nbx, oracle, monkeypatch):
    dim, n = 3, 257
    b, _, _ = system(oracle, dim, n, False)
    lib = nbx.load_library()
    NBX_ERR_INVALID, NBX_ERR_STATE = 1, 5
    t = np.arange(4, dtype=np.uint32)
    out = np.full((4, dim), 7.0)
    with nbx.Context(n, dim) as c:
        assert lib.nbx_ctx_compute_accel_active(c.h, t.ctypes.data, 4) == NBX_ERR_STATE          # nothing uploaded
        c.upload(b)
        assert lib.nbx_ctx_compute_accel_active(c.h, t.ctypes.data, 4) == NBX_ERR_STATE          # softening 0
        c.set_softening(EPS[False])
        assert lib.nbx_ctx_get_forces_active(c.h, oracle.G, out.ctypes.data) == NBX_ERR_STATE    # nothing computed yet
        assert lib.nbx_ctx_compute_accel_active(c.h, None, 4) == NBX_ERR_INVALID
        bad = np.array([0, n, 1], dtype=np.uint32)
        assert lib.nbx_ctx_compute_accel_active(c.h, bad.ctypes.data, 3) == NBX_ERR_INVALID and "n_total" in lib.nbx_last_error_detail().decode()
        assert lib.nbx_ctx_get_forces_active(c.h, oracle.G, out.ctypes.data) == NBX_ERR_STATE and (out == 7.0).all()
        c.compute_accel_active(t)
        assert lib.nbx_ctx_get_forces_active(c.h, oracle.G, None) == NBX_ERR_INVALID
        c.compute_accel_active([])                                                                 # an empty list is legal
        assert c.forces_active(oracle.G).shape == (0, dim)
        c.upload(b)                                                                                # an upload ends the sums' validity
        assert lib.nbx_ctx_get_forces_active(c.h, oracle.G, out.ctypes.data) == NBX_ERR_STATE
        heavy = b.copy()
        heavy[:, -1] *= 1.0e9                                                                      # masses up to 1e17 over eps^4 = 1e-24:
        c.upload(heavy)
        c.set_softening(1.0e-6)                                                                    # m / eps^4 out of fp32 range, nbx_ctx_compute_accel's rule
        assert lib.nbx_ctx_compute_accel_active(c.h, t.ctypes.data, 4) == lib.nbx_ctx_compute_accel(c.h, 0) == NBX_ERR_INVALID
    with nbx.Context(n, dim, n_shards=2, shard=0) as c:
        c.upload(b)
        c.set_softening(EPS[False])
        assert lib.nbx_ctx_compute_accel_active(c.h, t.ctypes.data, 4) == NBX_ERR_STATE
