"""Static check of the kernel of the digests of many nonces (csrc/md5_digest_many.hip
digest_many_kernel; no GPU needed): finding each entry's task on the device and one pass per task of a
wave cost it no scratch, no dynamic stack, no spilled VGPR and no AGPR -- no message word is indexed
at run time and no lane keeps a task row of its own -- and not the batch kernel's occupancy, by the
compiler's kernel resource remarks."""
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
    tmp = tmp_path_factory.mktemp("isa_digest_many")
    return {unit: _remarks(tmp, unit) for unit in ("md5_digest_many", "md5_batch")}


def _kernel_block(remarks, name):
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    mine = [b for b in blocks if name in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks]
    return mine[0]


def _figure(block, key):
    m = re.search(re.escape(key) + r": (\d+)", block)
    assert m, (key, block)
    return int(m.group(1))


def test_the_unit_has_one_kernel(remarks):
    blocks = re.split(r"remark: Function Name: ", remarks["md5_digest_many"])[1:]
    assert len(blocks) == 1 and "digest_many_kernel" in blocks[0].splitlines()[0]


def test_digest_many_kernel_uses_no_scratch(remarks):
    block = _kernel_block(remarks["md5_digest_many"], "digest_many_kernel")
    assert _figure(block, "ScratchSize [bytes/lane]") == 0, block
    assert "Dynamic Stack: False" in block
    assert re.search(r"VGPRs Spill: 0\b", block), block
    assert _figure(block, "AGPRs") == 0, block


def test_digest_many_kernel_keeps_the_batch_kernels_occupancy(remarks):
    d = _kernel_block(remarks["md5_digest_many"], "digest_many_kernel")
    b = _kernel_block(remarks["md5_batch"], "batch_kernel")
    for key in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"):
        print(key, "digest_many", _figure(d, key), "batch", _figure(b, key))
    assert _figure(d, "Occupancy [waves/SIMD]") >= _figure(b, "Occupancy [waves/SIMD]")
