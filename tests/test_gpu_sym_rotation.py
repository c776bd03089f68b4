"""GPU: the two rotations of the symmetric own-shard pass (csrc/force_sym_kernel.hip).  The default variant sympk3l_t8_w3
reads the visitors' {x, y, z, m} from a wave-private LDS buffer; the comparator sympk3l_t8_w3_dpp moves them from lane to
lane as the kernel did before.  Both feed the same values to the same arithmetic in the same order, so everything a launch
leaves behind must be equal BIT FOR BIT: the raw fp32 accelerations, the fp64 forces and, in mixed mode, the Q sums -- for
every shard shape the decomposition (csrc/sym_plan.h) distinguishes, with a planted sub-threshold pair so that the close
set's replacement of a body's planes runs, and for the same launch repeated."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LDS, DPP = "sympk3l_t8_w3", "sympk3l_t8_w3_dpp"

# super-blocks of 8,192 bodies: 2 (only the antipodal block); 3 with a ragged last one; 8 (even, four reaction slots);
# 9 (odd) and 10 (even) above 8; 128 = the benchmark's size
SIZES = (16384, 20480, 65536, 73728, 81920, 1 << 20)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.size} values differ"


def _evaluate(c, mixed):
    c.compute_accel()
    out = {"accel": c.accel(), "forces": c.forces()}
    if mixed:
        out["Q"] = c.aux()
    return out


@pytest.mark.parametrize("dim", (3, 2))
@pytest.mark.parametrize("n", SIZES)
def test_lds_rotation_equals_dpp_rotation_bit_for_bit(nbx, oracle, n, dim):
    names = nbx.variants()
    assert LDS in names and DPP in names, names
    assert names.index(DPP) == len(names) - 1, "the comparator is the table's last entry: no other index moved"
    b = oracle.generate(300 + dim, n, dim)
    # one pair at r^2 = 2.3e-13 (below the reference's skip threshold 1e-10), in different super-blocks: both bodies are
    # close-set targets and all their planes are replaced by the guarded evaluation
    far = np.full(dim - 1, 5.0e6)
    b[200, :dim] = np.concatenate(([3.0], far))
    b[n - 4000, :dim] = np.concatenate(([3.0 + 4.8e-7], far))
    b = oracle.round_inputs_to_f32(b)
    with nbx.Context(n, dim) as c:
        c.upload(b)
        for mixed in (False, True):
            c.set_refine(1.0e-5 if mixed else 0.0)
            got = {}
            for name in (LDS, DPP):
                c.set_tuning(0, names.index(name))
                assert c.effective_tuning()[0] == name, "both names must launch the symmetric pass here"
                first, second = _evaluate(c, mixed), _evaluate(c, mixed)
                for k in first:
                    assert k == "Q" or np.isfinite(first[k]).all(), (name, k)   # a close-set target's Q is +inf by design
                    _same(first[k], second[k], f"{name} N={n} D={dim} mixed={mixed}: {k}, the same launch twice")
                got[name] = first
            for k in got[LDS]:
                _same(got[LDS][k], got[DPP][k], f"N={n} D={dim} mixed={mixed}: {k}, LDS rotation against DPP rotation")
            assert np.abs(got[LDS]["accel"]).max() > 0.0


def test_comparator_is_never_a_default(nbx, oracle):
    names = nbx.variants()
    assert LDS in names and DPP in names, names
    for n, want in ((4096, None), (65536, LDS)):
        with nbx.Context(n, 3) as c:
            c.upload(oracle.round_inputs_to_f32(oracle.generate(9, n, 3)))
            name = c.effective_tuning()[0]
            assert name != DPP and (want is None or name == want), name
