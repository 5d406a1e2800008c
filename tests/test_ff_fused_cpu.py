"""The opt-in fused feed-forward kernel (mrag_ff_fused_bf16, layers.set_ff_fusion) without a GPU: its three entry points are declared, exported
and bound at ABI 11; the launch counter answers without a device; the argument checks return before any launch (so they are called here over made-up,
never dereferenced addresses) and a refused call does not count; ops.ff_fused_supported says what the header says; layers.set_ff_fusion marks exactly
the FeedForward modules and validates its argument."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_ff_fused_bf16", "mrag_ff_fused_supported", "mrag_ff_fused_launch_counts")


def test_ff_fused_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name
    assert "ff_fused.hip" in _lib.SOURCES
    assert L.mrag_ff_fused_bf16.argtypes == [ctypes.c_void_p, ctypes.POINTER(_lib.FfFusedArgs)]
    assert [f[0] for f in _lib.FfFusedArgs._fields_] == ["x", "out", "ln_gamma", "ln_beta", "w1", "b1", "w2", "b2", "rows", "C", "inner", "ldx", "ldo", "eps"]
    assert _lib.ABI_VERSION == 11 and L.mrag_abi_version() == 11          # added entry points do not move the ABI version
    assert "lvdm/modules/attention.py:448-475" in hdr                      # the reference call site is cited beside the declaration
    m = re.search(r"#define MRAG_FF_FUSED_ROWS (\d+)", hdr)
    from motionrag_amd import ops
    assert m and int(m.group(1)) == ops.FF_FUSED_ROWS


def test_ff_fused_counter_answers_without_a_device():
    from motionrag_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 2)(1 << 63, 1 << 63)
    assert L.mrag_ff_fused_launch_counts(buf, 2) == 1 and buf[0] < (1 << 63) and buf[1] == 1 << 63     # one slot, at most n written
    assert L.mrag_ff_fused_launch_counts(None, 0) == 1
    keep = (ctypes.c_uint64 * 1)(1 << 63)
    assert L.mrag_ff_fused_launch_counts(keep, 0) == 1 and keep[0] == 1 << 63
    # enum mrag_kernel_id and mrag_dispatch_counts stay as they are: the new kernel has no slot in the dispatch table
    n = L.mrag_dispatch_counts(None, 0)
    assert all(b"ff_fused" not in L.mrag_dispatch_name(i) for i in range(n))


def _args(**over):
    """a well-formed argument block over made-up (aligned, never dereferenced) device addresses"""
    from motionrag_amd import _lib
    a = _lib.FfFusedArgs()
    a.x, a.out, a.w1, a.w2 = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    a.ln_gamma, a.ln_beta, a.b1, a.b2 = 0x50000000, 0x50001000, 0x50002000, 0x50003000
    a.rows, a.C, a.inner, a.ldx, a.ldo, a.eps = 300, 320, 1280, 320, 320, 1e-5
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _count(L):
    buf = (ctypes.c_uint64 * 1)()
    L.mrag_ff_fused_launch_counts(buf, 1)
    return int(buf[0])


def test_ff_fused_argument_checks_return_before_any_launch():
    from motionrag_amd import _lib
    L = _lib.lib()
    call = lambda a: L.mrag_ff_fused_bf16(None, ctypes.byref(a))
    before = _count(L)
    assert L.mrag_ff_fused_bf16(None, None) == _lib.MRAG_EINVAL
    for C in (256, 640):
        assert call(_args(C=C, ldx=C, ldo=C)) == _lib.MRAG_ENOTSUP, C             # a shape outside the contract
    for inner in (96, 0, 32, -64):
        assert call(_args(inner=inner)) == _lib.MRAG_ENOTSUP, inner
    for field in ("x", "out", "w1", "w2"):
        assert call(_args(**{field: None})) == _lib.MRAG_EINVAL, field             # null required pointer
        assert call(_args(**{field: getattr(_args(), field) + 8})) == _lib.MRAG_EINVAL, field   # rows not 16-byte aligned
    for field in ("ln_gamma", "ln_beta", "b1", "b2"):
        assert call(_args(**{field: getattr(_args(), field) + 2})) == _lib.MRAG_EINVAL, field
    assert call(_args(ldx=324)) == _lib.MRAG_EINVAL                               # a row stride that is no multiple of 8 elements
    assert call(_args(ldo=312)) == _lib.MRAG_EINVAL                               # ... or below 320
    assert call(_args(ldx=312)) == _lib.MRAG_EINVAL
    assert call(_args(rows=0)) == _lib.MRAG_EINVAL
    assert call(_args(rows=-5)) == _lib.MRAG_EINVAL
    x = _args().x
    assert call(_args(out=x)) == _lib.MRAG_EINVAL                                 # out is x
    assert call(_args(out=x + 299 * 640 + 320)) == _lib.MRAG_EINVAL               # out starts inside x's last row
    assert call(_args(out=x + 160 * 640, ldo=328)) == _lib.MRAG_EINVAL            # out inside x's extent
    assert call(_args(x=x + 640, out=x, rows=2)) == _lib.MRAG_EINVAL              # x starts inside out's extent
    assert _count(L) == before                                                    # none of the refused calls counted as a launch


def test_ff_fused_supported_says_what_the_header_says_and_refuses_cpu_tensors():
    from motionrag_amd import _lib, ops
    L = _lib.lib()
    # include/mrag_hip.h, mrag_ff_fused_bf16: "MRAG_ENOTSUP unless C == 320, inner % 64 == 0 and 64 <= inner <= 2^20"
    hdr_says = lambda C, inner: C == 320 and inner % 64 == 0 and 64 <= inner <= (1 << 20)
    cases = [(320, 1280), (320, 64), (320, 128), (320, 192), (320, 1 << 20), (320, (1 << 20) + 64), (320, 96), (320, 0), (320, 32), (320, -64), (320, 1000),
             (256, 1280), (640, 2560), (1280, 5120), (64, 256), (0, 64), (328, 1280)]
    for C, inner in cases:
        assert ops.ff_fused_supported(C, inner) == hdr_says(C, inner), (C, inner)
        assert bool(L.mrag_ff_fused_supported(C, inner)) == hdr_says(C, inner), (C, inner)
    x = torch.zeros(4, 320, dtype=torch.bfloat16)
    w1, w2 = torch.zeros(128, 320, dtype=torch.bfloat16), torch.zeros(320, 64, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.ff_fused(x, None, None, 1e-5, w1, None, w2, None)


def _small_blocks():
    from motionrag_amd import dynamicrafter, svd_unet
    dc = dynamicrafter.BasicTransformerBlock(64, 1, 64, context_dim=64)
    sv = svd_unet.TemporalBasicTransformerBlock(64, 64, 1, 64, 64)
    return dc, sv


def test_set_ff_fusion_marks_the_feedforwards_and_validates():
    from torch import nn
    from motionrag_amd import dynamicrafter, layers, svd_unet
    dc, sv = _small_blocks()
    both = nn.ModuleList([dc, sv])
    ffs = [m for m in both.modules() if isinstance(m, (dynamicrafter.FeedForward, svd_unet.FeedForward))]
    assert len(ffs) == 3 and {id(m) for m in ffs} == {id(dc.ff), id(sv.ff_in), id(sv.ff)}
    marked = lambda: {id(m): getattr(m, layers.FF_FUSION_ATTR) for m in both.modules() if hasattr(m, layers.FF_FUSION_ATTR)}
    assert marked() == {}                                                         # a fresh model: nothing is marked
    for bad in ("on", 1, 0, None, "fp8"):
        with pytest.raises(ValueError):
            layers.set_ff_fusion(both, bad)
    assert marked() == {}                                                         # a refused call changes nothing
    assert layers.set_ff_fusion(both) is both
    assert marked() == {id(m): True for m in ffs}                                 # exactly the FeedForward modules
    layers.set_ff_fusion(dc, False)
    assert getattr(dc.ff, layers.FF_FUSION_ATTR) is False and getattr(sv.ff, layers.FF_FUSION_ATTR) is True
    layers.set_ff_fusion(both, False)
    assert marked() == {id(m): False for m in ffs}
    other, _ = _small_blocks()
    layers.set_ff_fusion(both, True)
    assert not hasattr(other.ff, layers.FF_FUSION_ATTR)                           # per module, not per class
    assert layers.FF_FUSION_ATTR != layers.FF_SITES_ATTR                          # an attribute of its own: the fp8 marks are untouched
    assert not any(hasattr(m, layers.FF_SITES_ATTR) for m in both.modules())
    assert isinstance(layers.FF_FUSED_MIN_ROWS, int) and layers.FF_FUSED_MIN_ROWS > 0
