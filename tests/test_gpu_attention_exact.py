"""Unmasked attention key by key: every kernel family behind ops.attention / attention_varlen / attention_small / the two fp8 entry points, on inputs whose
exact result is known (attn_exact.py; that they can fail is proven on the host in test_attn_exact_cpu.py).

Family A (every key counted exactly once; closed form n_d / L; three score levels 0, -20 and -90 nats) is judged at bf16's own rounding, |got - want| <=
2^-8 |want|; family B (every row, head and batch routed, K paired with its own V; fp64 softmax on the same inputs, leak asserted below 2^-12 before the
launch) at 2^-8 |want| + 2^-11.  Every element is counted.  K and V sit between guard rows (K = 0: score 0 against -20 / -90 nats; V = 1000), the result
inside a sentinel-filled buffer whose other rows and columns must keep the sentinel.  Every launch goes through ops.* inside ops.dispatched() and the exact
launch counters are asserted, so a case cannot land on another kernel family.

Each check prints `EXACT <case> <worst error as a fraction of its bound>` (pytest -s shows it); the bounds themselves are the derived ones."""
import pytest
import torch

import attn_exact as X
from test_gpu_attention_masked import PATH_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLIT_SHAPE = (2, 128, 1124, 1500)
SPLIT_BOUNDS = (512, 1024, 768)      # chunk boundaries of the two plans below: 3 chunks of 512 / 512 / 476 keys (attn16), 2 of 768 / 732 (32x32x16 family)


class tuned:
    """ops.TUNING["attn"] / ["attn_no_split"] for one block"""

    def __init__(self, tuning=0, no_split=False):
        self.new = {"attn": tuning, "attn_no_split": no_split}

    def __enter__(self):
        from motionrag_amd import ops
        self.old = {n: ops.TUNING[n] for n in self.new}
        ops.TUNING.update(self.new)

    def __exit__(self, *exc):
        from motionrag_amd import ops
        ops.TUNING.update(self.old)
        return False


def launch(q, k, v, want, tol, what, counts, *, tuning=0, no_split=False, layout="plain", kv_div=1, resid=False, entry="attention", **kw):
    """one launch of `entry` on guarded inputs into a sentinel-framed result: the counters, the frame, every element against `want` -> the worst error as a
    fraction of its bound.  resid: added in place with out_scale 0.5 (values in steps of 1/4), the bound then applies on the sum (attn_exact.py)"""
    from motionrag_amd import ops
    B, Sq, H, D = q.shape
    if layout == "fused":
        qd, kd, vd = X.fused_qkv(q, k, v, DEV)
        assert qd.stride(1) == 3 * H * D
    elif layout == "temporal":
        qd, kd, vd = X.temporal_qkv(q, k, v, DEV)
        assert qd.stride(0) == H * D and kd.stride(0) == 2 * H * D
    else:
        qd, (kd, vd) = q.to(DEV), X.guarded_kv(k, v, DEV)
    extra = None
    want = want.to(DEV)
    if resid:
        r = X.resid_values(B, Sq, H * D)
        ob = X.OutBuffer(B, Sq, H * D, DEV, fill=X.bf(r), temporal=layout == "temporal")
        kw.update(resid=ob.view, out_scale=0.5)
        extra = 2.0 ** -22 * (0.5 * want).abs()
        want = r.to(DEV).double() + 0.5 * want
    else:
        ob = X.OutBuffer(B, Sq, H * D, DEV, temporal=layout == "temporal")
    if kv_div != 1:
        kw["kv_batch_div"] = kv_div
    with tuned(tuning, no_split), ops.dispatched() as d:
        out = getattr(ops, entry)(qd, kd, vd, out=ob.view, **kw)
    assert d.counts == counts, (what, d.counts)
    assert out.data_ptr() == ob.view.data_ptr()
    assert ob.guards_intact(), f"{what}: a row or column outside the result was written"
    w = X.check(ob.view, want, what, extra=extra, **tol)
    print(f"EXACT {what} {w:.3g}")
    return w


def run_a(B, H, Sq, Skv, counts, what, D=64, prescaled=False, **kw):
    """family A at its three score levels"""
    X.check_shape_a(Skv, D)
    want = X.expected_a(B, H, Sq, Skv, D).to(DEV)
    if prescaled:                                    # Q is the constant itself: the scores stay uniform, `scale` is ignored
        kw.update(q_prescaled=True, scale=123.0)
    elif D != 64 or kw.get("entry") == "attention_small":
        kw["scale"] = 8.0 / D
    for q0 in X.Q0_LEVELS:
        q, k, v = X.family_a(B, H, Sq, Skv, q0, D, kv_div=kw.get("kv_div", 1))
        launch(q, k, v, want, X.TOL_A, f"A {what} s={8 * q0:g}", counts, **kw)


_B_CASES = {}


def case_b(B, H, Sq, Skv, D=64, kv_div=1, bounds=(), prescaled=False):
    """family B inputs (host) and their fp64 expected value (computed on the GPU, once per case, never written to); the leak condition is asserted here,
    before any launch"""
    key = (B, H, Sq, Skv, D, kv_div, bounds, prescaled)
    if key not in _B_CASES:
        q, k, v, pi = X.family_b(B, H, Sq, Skv, D, kv_div, boundaries=bounds)
        scale = 8.0 / D
        if prescaled:                                # the kernel takes these bf16 values as log2-unit scores; the expected value divides exactly them by log2 e
            q, scale = X.bf(q.float() * (X.LOG2E * scale)), 1.0 / X.LOG2E
        want, leak = X.ref64(q.to(DEV), k.to(DEV), v.to(DEV), scale, kv_div, pi)
        assert leak < X.LEAK, (key, leak)
        _B_CASES[key] = (q, k, v, want)
    return _B_CASES[key]


def run_b(B, H, Sq, Skv, counts, what, D=64, prescaled=False, bounds=(), **kw):
    q, k, v, want = case_b(B, H, Sq, Skv, D, kw.get("kv_div", 1), bounds, prescaled)
    if prescaled:
        kw.update(q_prescaled=True, scale=123.0)
    elif D != 64 or kw.get("entry") == "attention_small":
        kw["scale"] = 8.0 / D
    launch(q, k, v, want, X.TOL_B, f"B {what}", counts, **kw)


RUN = {"A": run_a, "B": run_b}
FAMILIES = ["A", "B"]


def shape_id(s):
    return "x".join(str(n) for n in s)


# ---------------------------------------------------------------------------------------------- 1. attn_tiny.hip
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape,kv_div,layout", [((3, 2, 16, 16), 1, "plain"), ((6, 2, 9, 5), 3, "temporal")], ids=["3x2x16x16", "6x2x9x5-kvdiv3-strided"])
def test_tiny(hip, family, shape, kv_div, layout):
    """one wavefront per (batch, head); the second shape with three query batches per K / V set on the (t, hw)-ordered views of the temporal transformers"""
    RUN[family](*shape, {"ATTN_TINY": 1}, f"tiny {shape_id(shape)}", kv_div=kv_div, layout=layout)


# ---------------------------------------------------------------------------------------------- 2. attn_flash.hip, unmasked
def flash_tuning(Sq, Skv):
    """unmasked launches of more than 128 rows over 256 keys or more go to attn16.hip unless the 32x32x16 family is asked for"""
    from motionrag_amd import ops
    return ops.ATTN_TUNE_LEGACY if Sq > 128 and Skv >= 256 else 0


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", PATH_SHAPES + [(2, 4, 385, 257), (1, 3, 200, 1000)], ids=shape_id)
def test_flash_unmasked(hip, family, shape):
    """the launch paths of test_gpu_attention_masked.py without a mask -- one, two and eight waves, the one-tile launch, Skv < 64 with clamped rows, the
    slid-back last tile -- and two long shapes on the 32x32x16 family (385 x 257 with B H = 8: the XCD block order; 1 000 keys: 15 ring stages and a ragged one)"""
    B, H, Sq, Skv = shape
    RUN[family](B, H, Sq, Skv, {"ATTN_FLASH": 1}, f"flash {shape_id(shape)}", tuning=flash_tuning(Sq, Skv))


# ---------------------------------------------------------------------------------------------- 3. attn16.hip
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", [(2, 3, 200, 256), (2, 4, 385, 257), (1, 3, 193, 1000), (1, 5, 600, 1343), (2, 2, 129, 1900)], ids=shape_id)
def test_attn16(hip, family, shape):
    """256 keys: four whole stages; 257: the last stage overlaps 63 keys of the one before, and B H = 8 takes the XCD block mapping; 193 rows: one full
    192-row workgroup and one row; 1 343 keys with B H = 5 (nbh & 7 != 0); 1 900: family A's longest key set.  At -90 nats the fast sweep's row sums fall
    below 2^-100 and the workgroup repeats the pass in the checked form"""
    B, H, Sq, Skv = shape
    RUN[family](B, H, Sq, Skv, {"ATTN16": 1}, f"attn16 {shape_id(shape)}")


# ---------------------------------------------------------------------------------------------- 4. the key-split tail and attn_combine_kernel
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kernels", ["attn16", "legacy"])
def test_key_split_tail(hip, family, kernels):
    """(2, 128, 1124, 1500).  attn16.hip: 5 full 192-row tiles and 164 rows whose keys go to chunks of 512 / 512 / 476 (the last one's own last tile slid back);
    32x32x16 family: 4 full 256-row tiles and 100 rows, chunks of 768 / 732.  The counters and a non-zero workspace are the check that the split route ran;
    the same expected values judge the launch with the split switched off"""
    from motionrag_amd import ops, _lib
    B, H, Sq, Skv = SPLIT_SHAPE
    assert _lib.lib().mrag_attn_workspace_bytes(B, H, Sq, Skv) > 0
    tuning = ops.ATTN_TUNE_LEGACY if kernels == "legacy" else 0
    split = {"ATTN_FLASH_KSPLIT": 1, "ATTN_COMBINE": 1} if kernels == "legacy" else {"ATTN16_KSPLIT": 1, "ATTN_COMBINE": 1}
    plain = {"ATTN_FLASH": 1} if kernels == "legacy" else {"ATTN16": 1}
    extra = {"bounds": SPLIT_BOUNDS} if family == "B" else {}
    RUN[family](B, H, Sq, Skv, split, f"ksplit {kernels}", tuning=tuning, **extra)
    RUN[family](B, H, Sq, Skv, plain, f"ksplit {kernels} no_split", tuning=tuning, no_split=True, **extra)


# ---------------------------------------------------------------------------------------------- 5. the fused features
FEATURES = {"fused_qkv": dict(layout="fused"), "kv_batch_div": dict(kv_div=2), "resid_in_place": dict(resid=True), "q_prescaled": dict(prescaled=True)}


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("feature", list(FEATURES))
@pytest.mark.parametrize("S,counts", [(321, {"ATTN16": 1}), (100, {"ATTN_FLASH": 1})], ids=["attn16-321", "flash-100"])
def test_features(hip, family, feature, S, counts):
    """strided views of one fused [B, S, 3, H, 64] buffer; two query batches per K / V set; resid + 0.5 * attention in place; a Q that already carries
    scale * log2 e -- each on an attn16 launch (321 x 321: ragged query tile, slid-back last stage) and a two-wave 32x32x16 launch (100 x 100)"""
    B = 4 if feature == "kv_batch_div" else 2
    RUN[family](B, 3, S, S, counts, f"{feature} {S}", **FEATURES[feature])


# ---------------------------------------------------------------------------------------------- 6. attn_varlen.hip
LENGTHS = [1, 63, 64, 65, 130, 0, 200, 257]


def varlen_launch(q, k, v, want, tol, what):
    from motionrag_amd import ops
    T, H = q.shape[0], q.shape[1]
    qd, kd, vd = X.packed_qkv(q, k, v, DEV)
    cu = torch.tensor([sum(LENGTHS[:i]) for i in range(len(LENGTHS) + 1)], dtype=torch.int32, device=DEV)
    buf = torch.full((X.ROW_PAD + T + 64, H * 64 + 2 * X.COL_PAD), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    out = buf[X.ROW_PAD:, X.COL_PAD:X.COL_PAD + H * 64]            # [T + 64, H * 64]: rows at or beyond cu_seqlens[-1] keep the sentinel
    before = ops.attn_varlen_launch_counts()
    with ops.dispatched() as d:
        res = ops.attention_varlen(qd, kd, vd, cu, max(LENGTHS), out=out)
    assert res is out and d.counts == {} and ops.attn_varlen_launch_counts() == before + 1
    rest = buf.clone()
    rest[X.ROW_PAD:X.ROW_PAD + T, X.COL_PAD:X.COL_PAD + H * 64] = X.SENTINEL
    assert (rest == X.SENTINEL).all(), f"{what}: a row or column outside the result was written"
    w = X.check(out[:T], want.to(DEV), what, **tol)
    print(f"EXACT {what} {w:.3g}")


@pytest.mark.parametrize("family", FAMILIES)
def test_varlen(hip, family):
    """one packed buffer, lengths on every side of the 64-key tile (clamped rows below 64 keys, the slid-back tile above), a 1-key and an empty sequence.
    Family A: n_d and L per sequence; the neighbouring sequences are each other's guard rows.  Family B: pi stays inside the row's own sequence"""
    if family == "A":
        for L in LENGTHS:
            X.check_shape_a(L)
        for q0 in X.Q0_LEVELS:
            q, k, v, want = X.packed_a(LENGTHS, 3, q0)
            varlen_launch(q, k, v, want, X.TOL_A, f"A varlen s={8 * q0:g}")
    else:
        q, k, v, want, leak = X.packed_b(LENGTHS, 3)
        assert leak < X.LEAK
        varlen_launch(q, k, v, want, X.TOL_B, "B varlen")


# ---------------------------------------------------------------------------------------------- 7. attn_small.hip
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", [32, 80, 96, 128])
def test_small_head_dims(hip, family, D):
    """300 rows: a second pass of the 256-thread row loop; 70 keys: four 16-key blocks and a ragged one of 6.  Moduli D / 2 - 1 and D / 2 + 1, scale 8 / D"""
    RUN[family](2, 3, 300, 70, {"ATTN_SMALL": 1}, f"small D={D}", D=D, entry="attention_small")


# ---------------------------------------------------------------------------------------------- 8. attn_fp8.hip
@pytest.mark.parametrize("entry,shape,prescaled", [("attention", (1, 2, 192, 512), False), ("joint_attention_fp8", (1, 2, 192, 600), False),
                                                   ("joint_attention_fp8", (1, 2, 192, 600), True)], ids=["fwd_fp8-512", "joint-600", "joint-600-prescaled"])
def test_fp8_family_a(hip, entry, shape, prescaled):
    """Family A alone, at bf16's bound, although the operands are e4m3: on these inputs nothing the format rounds differs between the keys of a row.  Q is one
    constant and K is +1 everywhere, so whatever their per-head power-of-two scales and e4m3 roundings make of them, every score of a row is the same number and
    P' = exp2(S' - m) * 8, rounded to e4m3, is ONE value for all keys.  V in {0, 1} has amax 1, its scale is a power of two and 0 and 2^ev are e4m3 numbers: V8
    is exact.  The fp32 sums of at most 640 copies of one 4-bit significand are exact, numerator n_d P' 2^ev and row sum L P' alike, and P' and 2^ev cancel in O:
    the only rounding left is the bf16 output.  600 keys are padded to 640 inside and masked: at -20 nats one leaked zero padding key would score e^20 times a
    real key and take the row"""
    kw = {"fp8": True} if entry == "attention" else {}
    run_a(*shape, {"ATTN_FP8": 1}, f"fp8 {entry} {shape_id(shape)}{' prescaled' if prescaled else ''}", entry=entry, prescaled=prescaled, **kw)
