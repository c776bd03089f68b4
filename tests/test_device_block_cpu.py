"""CPU: device memory's bookkeeping (csrc/device_block.h) -- the parked-block pool under the leaf plans' and the contexts' policy, the
owning Block and carve -- compiled with g++ under AddressSanitizer and UBSan (sanitizers run on the CPU build only) and driven by a
counting allocator, without a GPU: which block is taken, which is evicted, what is freed and when (tests/device_block_check.cpp says
what is pinned).  That the library's objects really reuse their blocks is the GPU tests' business (tests/test_gpu_one_shot.py)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_policies_blocks_and_carve(tmp_path):
    exe = str(tmp_path / "device_block_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "device_block_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
