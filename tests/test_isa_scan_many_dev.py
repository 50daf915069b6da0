"""Static check of the batched device scan's kernels (csrc/md5_scan_many_dev.hip; no GPU needed), by
the compiler's kernel resource remarks as in test_isa_scan_dev.py: the unit has exactly its four
kernels, none uses scratch, spills a VGPR or touches an AGPR, and the bitmap sink does not cost
scan_many_mask_kernel the occupancy of scan_many_kernel, whose loop it shares."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-proof-of-work_amd", "csrc")

pytestmark = pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")

KERNELS = ("scan_many_mask_kernel", "scan_many_place_kernel", "scan_many_rows_kernel", "scan_many_depth_kernel")


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
    tmp = tmp_path_factory.mktemp("isa_scan_many_dev")
    return {unit: _remarks(tmp, unit) for unit in ("md5_scan_many_dev", "md5_scan_many")}


def _kernel_block(remarks, name):
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    mine = [b for b in blocks if name + "E" in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks]
    return mine[0]


def _figure(block, key):
    m = re.search(re.escape(key) + r": (\d+)", block)
    assert m, (key, block)
    return int(m.group(1))


def test_the_unit_has_exactly_its_kernels(remarks):
    blocks = re.split(r"remark: Function Name: ", remarks["md5_scan_many_dev"])[1:]
    assert len(blocks) == len(KERNELS)
    for k in KERNELS:
        _kernel_block(remarks["md5_scan_many_dev"], k)


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_uses_no_scratch(remarks, kernel):
    block = _kernel_block(remarks["md5_scan_many_dev"], kernel)
    assert _figure(block, "ScratchSize [bytes/lane]") == 0, block
    assert "Dynamic Stack: False" in block
    assert re.search(r"VGPRs Spill: 0\b", block), block
    assert _figure(block, "AGPRs") == 0, block


def test_mask_kernel_keeps_the_batched_scan_kernels_occupancy(remarks):
    """The loop is scan_many_kernel's with a compare and two selects for a sink: it must not cost occupancy."""
    s = _kernel_block(remarks["md5_scan_many_dev"], "scan_many_mask_kernel")
    b = _kernel_block(remarks["md5_scan_many"], "scan_many_kernel")
    for key in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"):
        print(key, "scan_many_mask", _figure(s, key), "scan_many", _figure(b, key))
    assert _figure(s, "Occupancy [waves/SIMD]") >= _figure(b, "Occupancy [waves/SIMD]")
