"""The opt-in fp8 (e4m3) 3x3 convolution without a GPU: its two entry points are declared, exported and bound; the argument checks of mrag_conv_fp8
return before any launch (so they can be called here with made-up addresses); ops.conv_fp8_supported says what the C gate says on a table of
shapes; layers.set_conv_precision validates its argument and marks the 3x3 nn.Conv2d modules only."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mrag_conv_fp8", "mrag_conv_fp8_launch_counts")
EPI_NONE, EPI_GELU_TANH, EPI_RESID = 0, 1, 3


def test_conv_fp8_symbols_declared_exported_and_bound():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    declared = set(re.findall(r"\b(mrag_[a-z0-9_]+)\s*\(", hdr))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(raw, name), name
    assert "conv_fp8.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 11 and _lib.lib().mrag_abi_version() == 11           # added entry points do not move the version
    body = re.search(r"typedef struct mrag_conv_fp8_args \{(.*?)\} mrag_conv_fp8_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.ConvFp8Args._fields_]
    # the counter answers without a device: one slot, and mrag_fp8_launch_counts keeps its two
    buf = (ctypes.c_uint64 * 2)(1 << 63, 1 << 63)
    assert _lib.lib().mrag_conv_fp8_launch_counts(buf, 2) == 1 and buf[0] < (1 << 63) and buf[1] == 1 << 63
    assert _lib.lib().mrag_conv_fp8_launch_counts(None, 0) == 1
    assert _lib.lib().mrag_fp8_launch_counts(None, 0) == 2


def _args(N=2, H=16, W=24, Cin=64, Cout=256, epilogue=EPI_NONE, **over):
    """a well-formed argument block over made-up (aligned, never dereferenced) device addresses"""
    from motionrag_amd import _lib
    a = _lib.ConvFp8Args()
    a.x8, a.W8, a.x_exp, a.w_exp, a.y = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    a.N, a.H, a.Wd, a.Cin, a.Cout, a.stride, a.epilogue = N, H, W, Cin, Cout, 1, epilogue
    for k, v in over.items():
        setattr(a, k, v)
    return a


# every call below is refused: (arguments, why).  The C gate's verdict on the shape alone, for the comparison with ops.conv_fp8_supported
REFUSED_EINVAL = [dict(x8=None), dict(W8=None), dict(x_exp=None), dict(w_exp=None), dict(y=None),       # null pointers
                  dict(x8=0x100008), dict(W8=0x200008), dict(x_exp=0x300002), dict(w_exp=0x400001),      # misaligned pointers
                  dict(y=0x500004), dict(bias=0x600004), dict(epilogue=EPI_RESID), dict(epilogue=EPI_RESID, resid=0x600004),
                  dict(N=0), dict(Cin=0), dict(H=-1)]
REFUSED_ENOTSUP = [dict(Cin=96), dict(Cin=32), dict(Cout=258), dict(Cout=4), dict(Cout=8), dict(Cin=320, Cout=4), dict(stride=2), dict(upsample=1), dict(stride=2, asym_pad=1), dict(t_taps=3),
                   dict(epilogue=EPI_GELU_TANH),
                   dict(N=1, H=2048, W=2048, Cin=512),          # the offset guard: 2 samples of 2^31 bytes
                   dict(N=1, H=1024, W=1024, Cin=1024),         # the offset guard: 2^31 bytes at two samples
                   dict(Cin=16384, Cout=32768),                 # the offset guard: a 2^32-byte weight
                   dict(N=1, H=40000, W=4), dict(N=1, H=4, W=40000),
                   dict(N=40000, H=256, W=256)]                 # 2^31 pixels and more: the exponents are indexed by pixel


def test_conv_fp8_argument_checks_return_before_any_launch():
    from motionrag_amd import _lib
    L = _lib.lib()
    call = lambda a: L.mrag_conv_fp8(None, ctypes.byref(a))
    before = (ctypes.c_uint64 * 1)()
    L.mrag_conv_fp8_launch_counts(before, 1)
    assert L.mrag_conv_fp8(None, None) == _lib.MRAG_EINVAL
    for bad in REFUSED_EINVAL:
        assert call(_args(**bad)) == _lib.MRAG_EINVAL, bad
    for bad in REFUSED_ENOTSUP:
        assert call(_args(**bad)) == _lib.MRAG_ENOTSUP, bad
    after = (ctypes.c_uint64 * 1)()
    L.mrag_conv_fp8_launch_counts(after, 1)
    assert after[0] == before[0]                                                  # none of the refused calls counted as a launch


def test_conv_fp8_supported_agrees_with_the_c_gate():
    """the C gate's verdict on a well-formed call of a refused shape is MRAG_ENOTSUP; on an admitted shape the call would launch, so the admitted side is
    stated from the header's rule and checked against the GPU in tests/test_gpu_conv_fp8.py"""
    from motionrag_amd import _lib, ops
    L = _lib.lib()
    for bad in REFUSED_ENOTSUP:
        if "epilogue" in bad:
            continue
        a = _args(**bad)
        assert L.mrag_conv_fp8(None, ctypes.byref(a)) == _lib.MRAG_ENOTSUP
        if a.asym_pad or a.t_taps:                                                # not arguments of the Python gate: layers.conv3x3 never passes them
            continue
        assert not ops.conv_fp8_supported(a.N, a.H, a.Wd, a.Cin, a.Cout, a.stride, bool(a.upsample)), bad
    # (N, H, W, Cin, Cout, stride, upsample) -> admitted, written out from the header's rule (the admitted rows launch on the GPU: tests/test_gpu_conv_fp8.py)
    table = [((32, 72, 128, 320, 320, 1, False), True), ((32, 36, 64, 640, 640, 1, False), True), ((32, 18, 32, 1280, 1280, 1, False), True),
             ((32, 9, 16, 1280, 1280, 1, False), True), ((2, 16, 24, 64, 256, 1, False), True), ((3, 24, 24, 128, 260, 1, False), True),
             ((1, 1, 1, 64, 12, 1, False), True), ((1, 576, 1024, 128, 128, 1, False), True), ((16, 576, 1024, 128, 128, 1, False), True),
             ((32, 72, 128, 320, 320, 2, False), False), ((32, 36, 64, 640, 640, 1, True), False), ((2, 16, 24, 8, 256, 1, False), False),
             ((2, 16, 24, 64, 3, 1, False), False), ((2, 16, 24, 96, 256, 1, False), False), ((1, 2048, 2048, 512, 64, 1, False), False),
             ((0, 16, 24, 64, 64, 1, False), False),
             ((32, 72, 128, 320, 4, 1, False), False), ((28, 72, 128, 320, 4, 1, False), False), ((1, 64, 64, 512, 8, 1, False), False)]   # conv_out of the UNets / VAE encoders
    for row, want in table:
        assert ops.conv_fp8_supported(*row) == want, row
    assert ops.conv_fp8_supported(32, 72, 128, 320, 320) and not ops.conv_fp8_supported(32, 72, 128, 320, 320, stride=2)


def test_conv_fp8_ops_refuse_cpu_tensors():
    from motionrag_amd import ops
    x = torch.zeros(1, 4, 4, 64, dtype=torch.bfloat16)
    with pytest.raises(ops.HipOnly):
        ops.conv_implicit_fp8(x, torch.zeros(8, 576, dtype=torch.uint8), torch.zeros(8, dtype=torch.int32), None)


def test_set_conv_precision_validates_and_marks_only_3x3_conv2d():
    from motionrag_amd import layers

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c3 = nn.Conv2d(64, 64, 3, padding=1)
            self.c3s = nn.Conv2d(64, 64, 3, stride=2, padding=1)            # marked (a 3x3 Conv2d); the shape gate keeps it bf16
            self.c1 = nn.Conv2d(64, 64, 1)
            self.c13 = nn.Conv2d(64, 64, (1, 3))
            self.t3 = nn.Conv3d(64, 64, (3, 1, 1), padding=(1, 0, 0))
            self.c3d = nn.Conv3d(64, 64, 3, padding=1)
            self.lin = nn.Linear(64, 64)
            self.inner = nn.Sequential(nn.GroupNorm(32, 64), nn.SiLU(), nn.Conv2d(64, 128, 3, padding=1))

    m = Net()
    attr = layers.CONV_PRECISION_ATTR
    assert not any(hasattr(x, attr) for x in m.modules())                   # a fresh model carries no mark: bf16
    with pytest.raises(ValueError):
        layers.set_conv_precision(m, "int8")
    with pytest.raises(ValueError):
        layers.set_conv_precision(m, "fp16")
    assert not any(hasattr(x, attr) for x in m.modules())                   # a refused call changes nothing
    assert layers.set_conv_precision(m, "fp8") is m
    marked = sorted(n for n, x in m.named_modules() if getattr(x, attr, None) == "fp8")
    assert marked == ["c3", "c3s", "inner.2"]
    assert not any(hasattr(x, attr) for x in (m.c1, m.c13, m.t3, m.c3d, m.lin))
    other = Net()
    assert not any(hasattr(x, attr) for x in other.modules())               # per module, not per class
    layers.set_conv_precision(m.inner, "bf16")                              # a sub-module alone
    assert getattr(m.inner[2], attr) == "bf16" and getattr(m.c3, attr) == "fp8"
    layers.set_conv_precision(m)                                            # the default is bf16
    assert all(getattr(x, attr) == "bf16" for x in (m.c3, m.c3s, m.inner[2]))
