"""The persistent four-wave GEMM (csrc/gemm_w4.hip: gemm_w4_kernel) keeps nothing in scratch memory.  A spilled register is reloaded by a vector-memory
load, and vmcnt is ONE in-order counter for loads and stores: a reload placed among the epilogue's stores makes the wave wait for its own store stream
(nine times per tile in the GELU instantiation before the next tile's first fragments were taken out of the epilogue's live set), and one placed at the
tile change drains the LDS-DMA ring.  tests/test_scratch_cpu.py guards the K loop only; here the compiler's own bookkeeping is read for the whole kernel:
the code-object metadata of every instantiation, compiled as tests/test_gemm_w4_isa_cpu.py compiles it -- no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_four_wave_gemm_spills_nothing(tmp_path):
    asm = tmp_path / "gemm.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", os.path.join(ROOT, "motionrag_amd", "csrc", "gemm_w4.hip"), "-o", str(asm)],
                   check=True, capture_output=True, timeout=300)
    meta = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", asm.read_text(), flags=re.S | re.M).group(1)
    kernels = {}
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:                # one YAML list item per kernel
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, flags=re.M).group(1)
        inst = re.search(r"gemm_w4_kernelILi(\d+)ELb([01])E", name)
        if inst:
            kernels[(int(inst.group(1)), int(inst.group(2)))] = {k: int(v) for k, v in re.findall(r"^\s*\.(vgpr_spill_count|private_segment_fixed_size|vgpr_count):\s*(\d+)", entry, flags=re.M)}
    # the DiT's epilogues (0: plain, also with per-sample weights; 1: GELU; 3: residual; 4: gate + residual; 7: qk-norm + RoPE) and the UNets' (6, 8: GEGLU)
    assert {e for e, _ in kernels} >= {0, 1, 3, 4, 6, 7, 8}, sorted(kernels)
    assert (0, 1) in kernels, "the per-sample-weights instantiation"
    for inst, f in sorted(kernels.items()):
        assert f["vgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (inst, f)
        assert f["vgpr_count"] == 512, (inst, f)                       # all 512 registers: 256 accumulators in AGPRs beside the fragments
