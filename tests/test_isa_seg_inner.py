"""Static checks of the segment-inner sweep kernel's gfx950 code (no GPU needed).

The segment-inner kernel (md5_search_si.h search_body_si, the "_si" unit) hashes a
wave-block once per 2^24-k segment from lane invariants computed once per wave-block: step
W0 whole, step W0 + 1's bitop3 and the three later K + M[W0] adds leave the per-candidate
work.  Its hash block -- one segment's hash of a wave-block, <1,1,0> with the D-equality
test -- must hold at most 494 - 14 + 4 VALU instructions (the index-ordered kernel's 494,
7 fewer per candidate, 4 allowed for loop bookkeeping), keep the hand-ordered pipeline and
its padding, carry no SGPR-spill traffic, and keep the claim atomic ahead of the hashing.
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not shutil.which("/opt/rocm/bin/hipcc"), reason="hipcc not available")


@pytest.fixture(scope="module")
def kernel_si():
    import isa_loop
    text = isa_loop.disasm(os.path.join(ROOT, "distributed-proof-of-work_amd", "csrc"), 1, 0, ["-DDPOW_VSI=1"])
    lines = isa_loop.kernel_lines(text, 1, 1, 0, 1)
    assert lines, "no segment-inner <1,1,0,eq> kernel in the unit"
    assert "sik" in text, "the unit's kernels live in their own namespace"
    return isa_loop, lines


def _hash_block(isa_loop, lines):
    blocks = isa_loop.hash_block_mix(lines)
    assert blocks, "no hash block found"
    return max(blocks, key=lambda b: sum(b[2].values()))


def test_hash_block_has_at_most_484_valu_and_no_spill(kernel_si):
    isa_loop, lines = kernel_si
    lo, hi, c = _hash_block(isa_loop, lines)
    valu = sum(v for k, v in c.items() if k.startswith("v_") and "lane" not in k)
    print(f"segment-inner <1,1,0,eq> hash block: {valu} VALU, {dict(c)}")
    assert valu <= 484, valu
    assert valu >= 470, valu  # still a whole MD5 of two candidates from step W0 + 1
    assert c.get("v_readlane_b32", 0) + c.get("v_writelane_b32", 0) == 0
    assert c.get("s_nop", 0) >= 200  # padding after rotates and add3s
    # the hoisted work is gone: 2 x (step W0's add3 + rotate, step W0 + 1's bitop3)
    assert c["v_alignbit_b32"] <= 120 and c["v_bitop3_b32"] <= 118 and c["v_add3_u32"] <= 114


def test_pipeline_order_and_padding(kernel_si):
    _, lines = kernel_si
    m = {"v_bitop3_b32": "F", "v_add_u32_e32": "F", "v_add3_u32": "H", "v_alignbit_b32": "H", "s_nop": "n"}
    seq = "".join(m.get(l.split()[0], ".") for l in lines if re.search(r"//\s*[0-9A-F]{6,}:", l)).replace(".", "")
    group = "FHnHnFHnFFHn"  # md5_hash.h DPOW_PIPE_BODY
    assert seq.count(group) >= 50, seq[:400]
    body = seq[seq.find(group):seq.rfind(group) + len(group)]
    assert "HF" not in body and "HH" not in body


def test_claim_atomic_issued_ahead_of_the_hash_block(kernel_si):
    """The next claim's atomic is issued before the claim's last wave-block is hashed and its
    result is read (readfirstlane) after the hash block."""
    isa_loop, lines = kernel_si
    hash_lo = min(b[0] for b in isa_loop.hash_block_mix(lines))
    ins = []
    for l in lines:
        m = re.search(r"//\s*([0-9A-F]{6,}):", l)
        if m:
            ins.append((int(m.group(1), 16), l.split("//")[0].strip()))
    base = ins[0][0]
    hidden = False
    for i, (a, text) in enumerate(ins):
        m = re.match(r"global_atomic_add_x2 v\[(\d+):(\d+)\]", text)
        if not m or a - base >= hash_lo:
            continue
        regs = {f"v{m.group(1)}", f"v{m.group(2)}"}
        for a2, t2 in ins[i + 1:]:
            if t2.startswith("v_readfirstlane_b32") and t2.split(",")[-1].strip() in regs:
                hidden |= a2 - base > hash_lo
                break
    assert hidden, "every claim atomic is waited for before the hash block"
