"""Static check of the batch kernel's gfx950 code (csrc/md5_batch.hip; no GPU needed): its message
words live in registers.  A message-word array indexed by a runtime value would land in scratch,
which the kernel resource remarks of the compiler show as a non-zero ScratchSize."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-proof-of-work_amd", "csrc")

pytestmark = pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_batch") / "md5_batch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-DDPOW_NC=2", "--offload-arch=gfx950",
                        "-munsafe-fp-atomics", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "md5_batch.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _kernel_block(remarks):
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    mine = [b for b in blocks if "batch_kernel" in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks]
    return mine[0]


def test_batch_kernel_uses_no_scratch(remarks):
    block = _kernel_block(remarks)
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
    assert m, block
    assert int(m.group(1)) == 0, block
    assert "Dynamic Stack: False" in block
    assert re.search(r"VGPRs Spill: 0\b", block), block


def test_batch_kernel_resource_figures_are_reported(remarks):
    block = _kernel_block(remarks)
    for key in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"):
        m = re.search(re.escape(key) + r": (\d+)", block)
        assert m, (key, block)
        print(key, m.group(1))
