"""Static check of the batched scan's kernel (csrc/md5_scan_many.hip scan_many_kernel; no GPU
needed), by tests/test_isa_census_many.py's method: like batch_kernel it keeps its message words in
registers -- no scratch, no dynamic stack, no spilled VGPR, no AGPR -- by the compiler's kernel
resource remarks, and the descriptor, the per-task depth and the hit sink do not cost it the batch
kernel's occupancy."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-proof-of-work_amd", "csrc")

pytestmark = pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")


def _remarks(tmp, unit):
    out = tmp / (unit + ".o")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-DDPOW_NC=2", "--offload-arch=gfx950",
                        "-munsafe-fp-atomics", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, unit + ".hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isa_scan_many")
    return {unit: _remarks(tmp, unit) for unit in ("md5_scan_many", "md5_batch")}


def _kernel_block(remarks, name):
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    mine = [b for b in blocks if name in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks]
    return mine[0]


def _figure(block, key):
    m = re.search(re.escape(key) + r": (\d+)", block)
    assert m, (key, block)
    return int(m.group(1))


def test_scan_many_kernel_uses_no_scratch(remarks):
    block = _kernel_block(remarks["md5_scan_many"], "scan_many_kernel")
    assert _figure(block, "ScratchSize [bytes/lane]") == 0, block
    assert "Dynamic Stack: False" in block
    assert re.search(r"VGPRs Spill: 0\b", block), block
    assert _figure(block, "AGPRs") == 0, block


def test_scan_many_kernel_keeps_the_batch_kernels_occupancy(remarks):
    m = _kernel_block(remarks["md5_scan_many"], "scan_many_kernel")
    b = _kernel_block(remarks["md5_batch"], "batch_kernel")
    for key in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
        print(key, "scan_many", _figure(m, key), "batch", _figure(b, key))
    assert _figure(m, "Occupancy [waves/SIMD]") >= _figure(b, "Occupancy [waves/SIMD]")
