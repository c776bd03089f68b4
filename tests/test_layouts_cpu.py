"""CPU: nbx_leaf_pair_forces checks the body stride on the host, before it asks for a device (include/nbody_hip.h: body_stride_bytes
= sizeof(Body<dim>), larger strides allowed).  A stride below sizeof(Body<dim>), not a multiple of 8, or 0 is NBX_ERR_INVALID on a box
without a GPU too, and leaves the caller's force array alone; a valid wider stride gets as far as the device (NO_DEVICE there).
The other entry points that take a stride need a context or a plan first: their refusals are tested in tests/test_gpu_layouts.py."""
import ctypes

import numpy as np
import pytest

NBX_ERR_INVALID = 1


def _no_gpu(nbx):
    try:
        return nbx.device_count() == 0
    except nbx.NbxError:
        return True


@pytest.mark.parametrize("dim", (3, 2))
def test_leaf_pair_stride_is_validated_before_the_device(nbx, dim):
    lib = nbx.load_library()
    n = 10
    body = (2 * dim + 1) * 8
    b = np.zeros((n, 32))                                     # 256-byte records: room for every stride tried below
    b[:, :dim] = np.arange(n * dim).reshape(n, dim)
    b[:, 2 * dim] = 1.0
    lo, lb, so, ss = (np.ascontiguousarray(a, dtype=np.uint32)
                      for a in (np.array([0, 5, 10]), np.arange(10), np.array([0, 1, 2]), np.array([0, 1])))

    def call(stride, out):
        return lib.nbx_leaf_pair_forces(b.ctypes.data, n, dim, stride, lo.ctypes.data, lb.ctypes.data, 2, so.ctypes.data, ss.ctypes.data,
                                        nbx.LAW_FMM_P2P, 1.0, 0, out.ctypes.data, None)

    for stride in (body - 8, body - 1, 57, 0, 1):
        out = np.full((n, dim), -7.0)
        assert call(stride, out) == NBX_ERR_INVALID, stride
        assert (out == -7.0).all(), f"stride {stride}: a refused call wrote the force array"
        assert b"stride" in lib.nbx_last_error_detail()
    if _no_gpu(nbx):
        for stride in (body, body + 8, body + 24, 256):
            rc = call(stride, np.zeros((n, dim)))
            assert rc in (2, 3) and rc != NBX_ERR_INVALID, (stride, rc)          # NO_DEVICE / HIP: accepted, then no CPU fallback


def test_header_states_the_shard_row_counts():
    """The context's per-shard exports are `count` rows (shard_len or fewer, possibly none): the header says so where a caller sizes
    the buffers, and states what nbx_ctx_accuracy returns for an empty shard."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"\s+", " ", open(os.path.join(root, "include", "nbody_hip.h")).read())
    assert "float[dim][count]" in txt and "float[dim][shard_len]" not in txt
    for decl in ("int nbx_ctx_get_forces(", "int nbx_ctx_accuracy(", "int nbx_ctx_get_accel(", "int nbx_ctx_get_aux("):
        at = txt.index(decl)
        comment = txt[txt.rindex("/*", 0, at):at]
        assert "count" in comment, decl
    at = txt.index("int nbx_ctx_accuracy(")
    assert "0.0" in txt[txt.rindex("/*", 0, at):at]
