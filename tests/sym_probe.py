"""Sparse-mass probe of the symmetric own-shard force pass (test infrastructure; used by tests/test_gpu_sym_large.py and checked
on the host by tests/test_sym_plan_cpu.py).

All masses are zero except H <= 64 heavy bodies, so every raw acceleration is a sum of at most H pair terms and a (home,
visitor) meeting that the kernel drops or doubles moves it by O(1/H) of itself -- five orders of magnitude above the bounds.
Every pair is evaluated once: a body meets a heavy body either as its visitor (the heavy body is at home: the reaction sums,
slots S .. S + K - 1) or as its home (the heavy body visits: slots 0 .. S - 1), so heavy bodies spread over the blocks, slices
and chunks of the decomposition exercise both sides of every body of the shard.

The decomposition is restated here from the rule in csrc/sym_plan.h WITHOUT the library, and the shapes of the shard sizes
above 2^20 bodies are written down as a table; the C++ header is pinned to both by tests/test_sym_plan_cpu.py."""
import numpy as np

SUPER, HOME_PASS, GROUP, CHUNK_GROUPS, MAX_SLOTS, WANT_GROUPS = 8192, 2048, 64, 4, 128, 4096
SKIP_R2 = 1.0e-10   # the reference's skip rule: a pair below this r^2 contributes nothing

# pad: (B, S, K, G, chunks per slice, workgroups, slots); None: no plan, the context keeps the one-sided kernel
TABLE = {
    1052672: (129, 16, 64, 8, 2, 2064, 80),      # ragged
    1064960: (130, 16, 65, 8, 2, 2080, 81),
    1851392: (226, 8, 113, 16, 4, 1808, 121),
    2035712: (249, 4, 124, 32, 8, 996, 128),     # ragged; 256 planes
    2048000: (250, 2, 125, 64, 16, 500, 127),
    2080768: (254, 1, 127, 128, 32, 254, 128),
    2088960: (255, 1, 127, 128, 32, 255, 128),   # the largest shard with a plan: 5.98 GiB of planes at D = 3
    2097152: None,
}
PADS = tuple(p for p, row in TABLE.items() if row is not None)
PAD_NO_PLAN = 2097152


def plan(pad):
    """dict(B, S, K, G, gc, chunks, workgroups, slots) of a padded shard, or None where there is no symmetric decomposition."""
    B = (pad + SUPER - 1) // SUPER
    K = B // 2
    if pad == 0 or pad % (SUPER // 2) != 0 or B < 2 or K + 1 > MAX_SLOTS:
        return None
    S = SUPER // GROUP
    while S > 1 and (S + K > MAX_SLOTS or B * S > WANT_GROUPS):
        S //= 2
    G = SUPER // (S * GROUP)
    gc = min(G, CHUNK_GROUPS)
    return dict(B=B, S=S, K=K, G=G, gc=gc, chunks=G // gc, workgroups=B * S, slots=S + K)


def body_count(pad):
    """N with ceil(N / 4096) * 4096 = pad and N no multiple of 4096: pad bodies exist, and a ragged last super-block stays ragged."""
    return pad - 1234


def where(pad, i):
    """(super-block, slice, chunk, home pass) of body i."""
    p = plan(pad)
    block, o = divmod(i, SUPER)
    length = SUPER // p["S"]
    return block, o // length, (o % length) // (p["gc"] * GROUP), o // HOME_PASS


def heavy_indices(pad, n):
    """Indices of the heavy bodies, sorted: in super-blocks 0, 1, K - 1, K, K + 1 and B - 1 (with B even, K and K + 1 are the
    antipodal partners of 0 and 1, and K - 1 that of B - 1; a ragged B - 1 is the half block) the first chunk, the second
    chunk (c >= 1) and the last chunk of one slice -- the slice differs from block to block: first, last, middle; in the last
    block, whose tail is pad bodies, among the slices and chunks that hold none -- and the last valid body n - 1."""
    p = plan(pad)
    B, S, K = p["B"], p["S"], p["K"]
    length, clen = SUPER // S, p["gc"] * GROUP
    out = {n - 1}
    blocks = tuple(dict.fromkeys((0, 1, K - 1, K, K + 1, B - 1)))
    for j, block in enumerate(blocks):
        valid = min(SUPER, n - block * SUPER)             # the last block ends at body n - 1: pad bodies carry no mass
        slices = max(1, valid // length)                  # slices without a pad body (S = 1, 2: the one that holds body n - 1)
        s = (0, slices - 1, slices // 2)[j % 3]
        base = block * SUPER + s * length
        last = min(p["chunks"], min(length, valid - s * length) // clen) - 1   # the slice's last chunk without a pad body
        assert last >= min(1, p["chunks"] - 1), (pad, block, s, last)
        for c, lane in ((0, 5), (min(1, last), 77), (last, clen - 1 - 3 * j)):
            i = base + c * clen + lane
            assert i < n, (pad, block, s, c, lane)
            out.add(i)
    assert len(out) == 3 * len(blocks) + 1, "no heavy body dropped or placed twice"
    return np.array(sorted(out), dtype=np.int64)


def coverage(pad, n, heavy):
    """Which features of the decomposition the heavy bodies reach, as a dict of booleans (asserted on the host and before the
    GPU probe): every chunk position of a slice, the blocks at both ends of the rotation, both kinds of slot."""
    p = plan(pad)
    at = [where(pad, int(i)) for i in heavy]
    blocks = {a[0] for a in at}
    want = {0, 1, p["K"], p["K"] + 1, p["B"] - 1} | ({p["K"] - 1} if p["B"] % 2 == 0 else set())
    passes = [(a[0], a[3]) for a in at]
    return dict(at_most_64=len(heavy) <= 64, first_chunk=any(a[2] == 0 for a in at), later_chunk=any(a[2] >= 1 for a in at),
                last_chunk=any(a[2] == p["chunks"] - 1 for a in at), blocks=want <= blocks, last_body=int(heavy[-1]) == n - 1,
                two_in_one_home_pass=len(set(passes)) < len(passes), first_and_last_slice={0, p["S"] - 1} <= {a[1] for a in at},
                more_than_one_chunk=p["chunks"] > 1,
                later_chunk_in_last_block=any(a[0] == p["B"] - 1 and a[2] >= 1 for a in at))


def sparse_bodies(oracle, seed, pad, dim):
    """(bodies rounded to fp32 with every mass but the heavy bodies' zero, heavy indices)."""
    n = body_count(pad)
    b = oracle.generate(seed, n, dim)
    heavy = heavy_indices(pad, n)
    m = b[heavy, -1].copy()
    b[:, -1] = 0.0
    b[heavy, -1] = m
    return oracle.round_inputs_to_f32(b), heavy


def reference(bodies, heavy):
    """fp64 numpy over the N x H pairs: (a [N, D] with a_i = sum_j m_j (p_j - p_i) / r^4, the magnitude sums sum_j |a_ij|)."""
    dim = (bodies.shape[1] - 1) // 2
    pos = np.ascontiguousarray(bodies[:, :dim])
    a, mag = np.zeros_like(pos), np.zeros(pos.shape[0])
    for j in heavy:
        d = pos[j] - pos
        r2 = (d * d).sum(axis=1)
        keep = r2 >= SKIP_R2                       # the body itself and the reference's skip rule
        w = np.where(keep, bodies[j, -1] / np.where(keep, r2 * r2, 1.0), 0.0)
        a += w[:, None] * d
        mag += w * np.sqrt(r2)
    return a, mag
