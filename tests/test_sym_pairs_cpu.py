"""The symmetric pass with two visitors per lane (D = 3), without a GPU: a CPU model of its summation order on both sides
(tests/sym_sum_model_pairs.cpp) on the input of tests/test_sym_plan_cpu.py's model test -- 65,536 uniform bodies, seed 2, the
fp64 reference checked against the oracle's rows.

What changes against the one-visitor form is the visitor's level 1 alone: one fp32 chain of 8 terms per step over a block of
steps instead of two half-chains added at the flush.  The model gives it for blocks of 8 steps (64 terms) and of 4 (32 terms).
Bounds, none taken from what the model gives (the same three as the existing model test):
  * backward error |dF_i| <= TOL_BACKWARD * S_i for every body (oracle_lib);
  * the sigma a body needs, |dF_i| / (u sqrt(Q_i)), among bodies over half of mixed mode's tolerance (1e-5): < 24, the frozen
    sigma factor of the three-level summation in 3D (tests/test_tolerances_frozen.py);
  * where no body is over half the tolerance, the same for EVERY body.
The home side keeps the one-visitor form's bits: the model holds both orders side by side and counts the level-1 and level-2
sums that differ; and its restatement of the one-visitor order is pinned to tests/sym_sum_model.cpp's output bit for bit.

The kernel flushes every 8 steps (kSymBlockSteps): the bounds hold for 8, so the shorter block with twice the flushes is not
needed.  The figures of both are printed for the record (profiles/r15/sym_two_visitors.txt)."""
import os
import re
import subprocess

import numpy as np

from oracle_lib import TOL_BACKWARD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA_3D = 24.0        # kRefineSigmaDefault3D, frozen
U32 = 2.0 ** -24
KERNEL_BLOCK_STEPS = 8


def _build(tmp_path, src):
    exe = str(tmp_path / os.path.splitext(src)[0])
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O2", "-fopenmp", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", src), "-o", exe], check=True)
    return exe


def _norm(a):
    return np.sqrt((a * a).sum(axis=1))


def test_summation_model_of_two_visitors_per_lane_at_65536_bodies(tmp_path, oracle):
    n, dim = 1 << 16, 3
    b = oracle.round_inputs_to_f32(oracle.generate(2, n, dim))
    src, dst, dst_old = tmp_path / "in.f32", tmp_path / "pairs.f64", tmp_path / "old.f64"
    np.ascontiguousarray(np.concatenate([b[:, :3], b[:, -1:]], axis=1), dtype=np.float32).tofile(src)
    p = subprocess.run([_build(tmp_path, "sym_sum_model_pairs.cpp"), str(src), str(dst), str(n)], check=True,
                       capture_output=True, text=True)
    subprocess.run([_build(tmp_path, "sym_sum_model.cpp"), str(src), str(dst_old), str(n), "32"], check=True)
    out = np.fromfile(dst, dtype=np.float64).reshape(n, 16)
    old = np.fromfile(dst_old, dtype=np.float64).reshape(n, 12)
    scale = -oracle.G * b[:, -1:]   # F_i = -(G m_i) a_i, the reference's sign
    ref, S = out[:, 0:3] * scale, out[:, 3] * np.abs(scale[:, 0])
    # the model's fp64 reference is the oracle's
    rows = np.arange(0, n, 257, dtype=np.int64)
    want = oracle.force_rows_omp_2(b, rows)
    assert np.abs(ref[rows] - want).max() <= 1e-12 * np.abs(want).max()

    # the home side: level-1 and level-2 sums (and Q) of the two-visitor order against the one-visitor order, bit for bit ...
    m = re.search(r"home_level1_differ=(\d+) home_level2_differ=(\d+)", p.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (0, 0), p.stdout
    # ... and the one-visitor order this model restates IS the existing model's: both sides, every body, Q included
    assert np.array_equal(out[:, 0:4], old[:, 0:4]) and np.array_equal(out[:, 4:8], old[:, 8:12])

    report = {}
    for name, col in (("one visitor per lane (existing model)", 4), ("two visitors, blocks of 8 steps", 8),
                      ("two visitors, blocks of 4 steps", 12)):
        f, Q = out[:, col:col + 3] * scale, out[:, col + 3] * scale[:, 0] ** 2
        d = _norm(f - ref)
        rel, back, need = d / _norm(ref), d / S, d / (U32 * np.sqrt(Q))
        over = rel > 0.5e-5
        report[name] = dict(max_backward=back.max(), max_rel=rel.max(), n_rel_gt_half_tol=int(over.sum()),
                            sigma_needed_max=need.max(), sigma_needed_p9999=np.percentile(need, 99.99),
                            sigma_needed_max_among_rel_gt_half_tol=need[over].max() if over.any() else 0.0)
        print(name, report[name])
    # the order changes the reaction sums only, and not in every bit of every body
    assert not np.array_equal(out[:, 8:11], out[:, 4:7])
    assert KERNEL_BLOCK_STEPS == 8
    for name in ("two visitors, blocks of 8 steps", "one visitor per lane (existing model)"):
        r = report[name]
        assert r["max_backward"] <= TOL_BACKWARD, (name, r)
        assert r["sigma_needed_max_among_rel_gt_half_tol"] < SIGMA_3D, (name, r)
        assert r["n_rel_gt_half_tol"] > 0 or r["sigma_needed_max"] < SIGMA_3D, (name, r)
