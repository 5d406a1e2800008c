"""The argument checks of the attention entry points without a GPU: mrag_attn_fwd_bf16, mrag_attn_fwd_fp8, mrag_attn_joint_fwd_fp8 and mrag_attn_small_bf16 take the
same mrag_attn_args block and refuse a malformed one before any launch, so each is called here with one violation over made-up (aligned, never dereferenced)
addresses and a null stream, and the literal status code is asserted -- the order in which MRAG_EINVAL and MRAG_ENOTSUP are decided included.  The fp8 entry
points' own refusals are in test_fp8_joint_attention_cpu.py; mrag_ip_attn_folded_bf16 (scalar arguments) has a few rows of its own."""
import ctypes
from contextlib import contextmanager

import pytest

Q0, O0, WS0, EXTRA = 0x1000000, 0x4000000, 0x8000000, 0x9000000       # Q (K, V follow inside one fused buffer), O, workspace, mask / bias / resid


def _args(B=1, H=2, Sq=300, Skv=513, D=64, ws=False, **over):
    """a well-formed block: q / k / v as views of one fused [B, S, 3, H, D] buffer, o [B, Sq, H * D]; `ws`: with the fp8 entry points' (required) scratch"""
    from motionrag_amd import _lib
    a = _lib.AttnArgs()
    S = max(Sq, Skv, 1)
    a.Q, a.K, a.V, a.O = Q0, Q0 + 2 * H * D, Q0 + 4 * H * D, O0
    a.q_sb = a.k_sb = a.v_sb = S * 3 * H * D
    a.q_ss = a.k_ss = a.v_ss = 3 * H * D
    a.q_sh = a.k_sh = a.v_sh = D
    a.o_sb, a.o_ss = max(Sq, 1) * H * D, H * D
    a.B, a.H, a.Sq, a.Skv, a.kv_batch_div = B, H, Sq, Skv, 1
    a.scale, a.out_scale = 0.125, 1.0
    if ws:
        a.workspace, a.workspace_bytes = WS0, 1 << 40
    for k, v in over.items():
        setattr(a, k, v)
    return a


@contextmanager
def _no_launch():
    """every case is a refusal: none of them may count as a launch"""
    from motionrag_amd import _lib
    L = _lib.lib()
    n = L.mrag_dispatch_counts(None, 0)
    before, after = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
    L.mrag_dispatch_counts(before, n)
    yield L
    L.mrag_dispatch_counts(after, n)
    assert list(after) == list(before)


def _entry(L, name):
    """name -> (call(args block), keyword arguments of a block the entry point would accept)"""
    if name == "small":
        return (lambda a, head_dim=32: L.mrag_attn_small_bf16(None, ctypes.byref(a), head_dim)), dict(D=32)
    if name == "bf16":
        return (lambda a: L.mrag_attn_fwd_bf16(None, ctypes.byref(a))), dict()
    if name == "fp8":
        return (lambda a: L.mrag_attn_fwd_fp8(None, ctypes.byref(a))), dict(Skv=640, ws=True)       # whole 128-key stages only
    return (lambda a: L.mrag_attn_joint_fwd_fp8(None, ctypes.byref(a))), dict(ws=True)


# one violation each, MRAG_EINVAL at all four entry points
COMMON = ([(f"{f} null", {f: None}) for f in ("Q", "K", "V", "O")] +
          [(f"{f} = {bad}", {f: bad}) for f in ("B", "H", "Sq", "Skv") for bad in (0, -3)] +
          [("Q misaligned by 8", {"Q": Q0 + 8}), ("K misaligned by 8", {"K": Q0 + 8}), ("V misaligned by 8", {"V": Q0 + 8}),
           ("q_ss % 8", {"q_ss": 388}), ("k_sh % 8", {"k_sh": 68}), ("v_sb % 8", {"v_sb": 513 * 384 + 4})])


@pytest.mark.parametrize("name", ["bf16", "fp8", "joint", "small"])
def test_common_argument_errors(name):
    from motionrag_amd import _lib
    with _no_launch() as L:
        call, base = _entry(L, name)
        raw = {"bf16": L.mrag_attn_fwd_bf16, "fp8": L.mrag_attn_fwd_fp8, "joint": L.mrag_attn_joint_fwd_fp8}.get(name)
        assert (raw(None, None) if raw else L.mrag_attn_small_bf16(None, None, 32)) == _lib.MRAG_EINVAL
        for what, over in COMMON:
            assert call(_args(**{**base, **over})) == _lib.MRAG_EINVAL, (name, what)


def test_bf16_entry_point_refusals():
    from motionrag_amd import _lib
    EINVAL, ENOTSUP = _lib.MRAG_EINVAL, _lib.MRAG_ENOTSUP
    with _no_launch() as L:
        call, _ = _entry(L, "bf16")
        for what, over, code in [
                ("O misaligned by 4", dict(O=O0 + 4), EINVAL),
                ("o_ss % 4", dict(o_ss=2 * 64 + 2), EINVAL),
                ("resid misaligned by 4", dict(resid=EXTRA + 4), EINVAL),
                ("kv_batch_div = 0", dict(kv_batch_div=0), EINVAL),
                ("B % kv_batch_div", dict(B=3, kv_batch_div=2), EINVAL),
                ("k_ss < 0", dict(k_ss=-8), ENOTSUP),                                  # the 32-bit K / V tile offsets of the LDS-DMA path
                ("k_ss too large", dict(k_ss=0x2000000), ENOTSUP),
                ("bias misaligned by 2", dict(bias=EXTRA + 2, bias_sh=300 * 513), EINVAL),
                ("bias_sh < 0", dict(bias=EXTRA, bias_sh=-1), EINVAL),
                ("key-split workspace misaligned by 8", dict(Sq=129, Skv=256, workspace=WS0 + 8, workspace_bytes=1 << 30), EINVAL),
                # precedence: the stride range is decided before the bias is looked at
                ("k_ss too large + misaligned bias", dict(k_ss=0x2000000, bias=EXTRA + 2, bias_sh=300 * 513), ENOTSUP)]:
            assert call(_args(**over)) == code, what


def test_fp8_entry_points_workspace_alignment_and_precedence():
    from motionrag_amd import _lib
    EINVAL, ENOTSUP = _lib.MRAG_EINVAL, _lib.MRAG_ENOTSUP
    with _no_launch() as L:
        for name in ("fp8", "joint"):
            call, base = _entry(L, name)
            assert call(_args(**{**base, "workspace": WS0 + 8})) == EINVAL, name
            assert call(_args(**base, mask=EXTRA, Q=Q0 + 8)) == ENOTSUP, name              # the refusals come before the alignment rules ...
        call, base = _entry(L, "fp8")
        assert call(_args(Skv=576)) == EINVAL                                              # ... and after the null checks, the workspace's included


def test_small_entry_point_refusals():
    from motionrag_amd import _lib
    EINVAL, ENOTSUP = _lib.MRAG_EINVAL, _lib.MRAG_ENOTSUP
    with _no_launch() as L:
        call, base = _entry(L, "small")
        for what, over, code in [
                ("O misaligned by 8", dict(O=O0 + 8), EINVAL),                          # 16-byte stores here (mrag_attn_fwd_bf16 stores 8 bytes and takes this O)
                ("o_ss % 8", dict(o_ss=2 * 32 + 4), EINVAL),
                ("mask", dict(mask=EXTRA), ENOTSUP),
                ("bias", dict(bias=EXTRA, bias_sh=300 * 513), ENOTSUP),
                ("resid", dict(resid=EXTRA), ENOTSUP),
                ("kv_batch_div = 2", dict(kv_batch_div=2), ENOTSUP),
                ("q_prescaled", dict(q_prescaled=1), ENOTSUP),
                ("mask + misaligned Q", dict(mask=EXTRA, Q=Q0 + 8), ENOTSUP)]:           # precedence: the refusals come before the alignment rules
            assert call(_args(**{**base, **over})) == code, what
        assert call(_args(D=64), 64) == ENOTSUP                                             # head dim 64 belongs to mrag_attn_fwd_bf16
        assert call(_args(D=128, Skv=257), 128) == ENOTSUP                                  # K and V of a head in LDS: 257 * 128 * 4 bytes > 128 KiB


def test_ip_attn_folded_refusals():
    from motionrag_amd import _lib
    with _no_launch() as L:
        def call(scores=Q0, v=O0, hidden=WS0, B=1, S=64, H=2, keys=25, kv_batch_div=1, scores_ld=64, hidden_ld=128, v_bs=25 * 128, v_ks=128, key_stride=32):
            return L.mrag_ip_attn_folded_bf16(None, scores, v, hidden, B, S, H, keys, kv_batch_div, scores_ld, hidden_ld, v_bs, v_ks, 0.125, 1.0, key_stride)
        assert call(keys=33) == _lib.MRAG_EINVAL
        assert call(scores_ld=68) == _lib.MRAG_EINVAL
        assert call(hidden=WS0 + 8) == _lib.MRAG_EINVAL
