"""The frame-parallel (tier 2) DynamiCrafter UNet with 2 and 4 ranks on ONE GPU: tools/frame_parallel_check.py started through torch.distributed.run as a
CHILD process (nothing here re-execs a process that touched the GPU; at most 5 processes hold the GPU: this one and four ranks), every rank on cuda:0,
collectives through gloo.  World 4 gives t_loc = 1 on the 4-frame fixture and a 4-pixel slab at the lower level: the smallest shape at which the frame
order, the slab split and the statistics gather can each go wrong.  The worker asserts and exits non-zero on the first failure; this parent asserts the
return code, reads the one JSON line and re-checks the asserted quantities.  Nothing is retried."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ranks(world):
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join("tools", "frame_parallel_check.py")], cwd=ROOT, env=dict(os.environ),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [l for l in out.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    print(f"world {world}: sharded vs golden {d['rel_fro_sharded_vs_golden']:.4e}, unsharded vs golden {d['rel_fro_unsharded_vs_golden']:.4e}, "
          f"sharded vs unsharded {d['rel_fro_sharded_vs_unsharded']:.4e}; GroupNorm launches of one sharded forward {d['launches']}")
    assert d["world"] == world and d["shape"] == [2, 4, 4, 8, 8] and d["finite"] and d["same_bits_on_all_ranks"] and d["repeatable"]
    assert d["rel_fro_sharded_vs_golden"] <= 3e-2                           # the bound of tests/test_gpu_unet.py::test_dc_unet_against_reference_golden
    # sharding only re-partitions fp32 statistic sums: it must cost less than the bf16 model's own distance from the fp32 oracle
    assert d["rel_fro_sharded_vs_unsharded"] <= d["rel_fro_unsharded_vs_golden"]
    return d


@pytest.mark.timeout(900)
def test_two_ranks_reproduce_the_unsharded_unet(hip):
    _ranks(2)


@pytest.mark.timeout(900)
def test_four_ranks_reproduce_the_unsharded_unet(hip):
    _ranks(4)
