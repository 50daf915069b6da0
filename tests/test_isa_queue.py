"""Static check of the task queue's kernel (csrc/md5_batch.hip queue_kernel; no GPU needed): like
batch_kernel it keeps its message words in registers -- no scratch, no spilled VGPR -- by the
compiler's kernel resource remarks."""
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
    out = tmp_path_factory.mktemp("isa_queue") / "md5_batch.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-DDPOW_NC=2", "--offload-arch=gfx950",
                        "-munsafe-fp-atomics", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "md5_batch.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _kernel_block(remarks, name):
    blocks = re.split(r"remark: Function Name: ", remarks)[1:]
    mine = [b for b in blocks if name in b.splitlines()[0]]
    assert len(mine) == 1, [b.splitlines()[0] for b in blocks]
    return mine[0]


@pytest.mark.parametrize("name", ["queue_kernel", "queue_upload_kernel"])
def test_queue_kernels_use_no_scratch(remarks, name):
    block = _kernel_block(remarks, name)
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block)
    assert m, block
    assert int(m.group(1)) == 0, block
    assert "Dynamic Stack: False" in block
    assert re.search(r"VGPRs Spill: 0\b", block), block


def test_queue_kernel_registers_match_the_batch_kernel(remarks):
    """Both entry points run the same BatchGroup: the queue's must not cost occupancy."""
    q, b = _kernel_block(remarks, "queue_kernel"), _kernel_block(remarks, "batch_kernel")
    fig = {}
    for key in ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"):
        mq, mb = (re.search(re.escape(key) + r": (\d+)", blk) for blk in (q, b))
        assert mq and mb, key
        fig[key] = (int(mq.group(1)), int(mb.group(1)))
        print(key, "queue", fig[key][0], "batch", fig[key][1])
    assert fig["Occupancy [waves/SIMD]"][0] >= fig["Occupancy [waves/SIMD]"][1]
