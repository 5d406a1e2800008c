"""The two softmax kernels that work on a materialised score matrix, key by key and column by column: ip_attn_folded_kernel (ops.ip_attn_folded_) and
softmax_rows_kernel (ops.softmax_rows) on inputs whose exact result is known (softmax_exact.py: families, bounds and their derivations; that every check
accepts a correct kernel's arithmetic and can fail is proven on the host in test_softmax_exact_cpu.py).

ip_attn_folded: the scores sit in a [B, S, W] buffer whose every other column is NaN (W once the narrowest the entry point admits, once 64 more), V is a
column block of a NaN-padded buffer, `hidden` carries the residual between 64 sentinel rows in front and behind that must survive, and every launch asserts
d.counts == {"IP_ATTN_FOLDED": 1}.  Family A at 2^-8 |want| + 2^-22 |out_scale n_d / keys|, family B with torch.equal, family G at its derived bound.
ops.ip_attn_folded_ asks for W >= (H - 1) ks + 32, the C ABI for ((H - 1) ks & ~7) + 32: where the first is more (ks no multiple of 8) the narrow launch
goes through the C ABI, as all of case 9 does.

softmax_rows: scale 512^-0.5, out of place and in place, two row strides, NaN in x's padding and guard rows, a sentinel in y's (in place: in the one
buffer's) that must survive.  Families C and P at 2^-8 (1 + 2^-10) want + 2^-40, family G at (2^-8 + 2^-16) want + 2^-40.

Each check prints `EXACT <case> <worst error as a fraction of its bound>` (pytest -s shows it); the bounds themselves are the derived ones.

Worst fractions measured on an MI355X, over all launches of a family (316 in all): ip_attn_folded A 0.828, B 0 (bit for bit), G 0.937 (the host emulation
of the kernel's rounding points: 0.94); softmax_rows C 0.500 (bf16(1/24) itself is 0.4995 x 2^-8 off 1/24), P 1.2e-12, P at 136 nats 1.2e-47, G 0.977
(emulation: 0.977).  No test found a fault in either kernel."""
import ctypes

import pytest
import torch

import softmax_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
IP_COUNTS = {"IP_ATTN_FOLDED": 1}


# ============================================================================================== ip_attn_folded
def ip_widths(case):
    """(W, through the C ABI) of a case's two launches"""
    H, keys, ks = X.IP_CASES[case][:3]
    c_min, ops_min = X.ip_min_width(H, ks, "c"), X.ip_min_width(H, ks, "ops")
    assert c_min >= (H - 1) * ks + keys
    return [(c_min, case == 9 or c_min < ops_min), (ops_min + 64, case == 9)]


def ip_launch(case, what, sc, v, r, out_scale, judge):
    """both widths of one input set: counters, guards, then `judge(result) -> worst fraction`"""
    from motionrag_amd import _lib, ops
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    worst = 0.0
    for W, c_abi in ip_widths(case):
        scores = X.ip_scores_buffer(sc, ks, W).to(DEV)
        vb = X.ip_v_buffer(v, DEV)
        hb = X.Hidden(r, DEV, col_pad=64 if case == 9 else 0)
        with ops.dispatched() as d:
            if c_abi:
                ptr = [ctypes.c_void_p(t.data_ptr()) for t in (scores, vb, hb.inner)]
                rc = _lib.lib().mrag_ip_attn_folded_bf16(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), *ptr, B, S, H, keys, kv_div, W, hb.ld,
                                                         vb.stride(0), vb.stride(1), X.IP_SCALE, out_scale, ks)
                assert rc == _lib.MRAG_OK, rc
            else:
                ops.ip_attn_folded_(scores, vb, hb.view, H, keys, kv_batch_div=kv_div, scale=X.IP_SCALE, out_scale=out_scale, key_stride=ks)
        assert d.counts == IP_COUNTS, (what, d.counts)
        assert hb.guards_intact(), f"{what}: a row or column outside `hidden` was written"
        w = judge(hb.result(), f"{what} W={W}")
        print(f"EXACT {what} W={W}{' C-ABI' if c_abi else ''} {w:.3g}")
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("case", list(X.IP_CASES))
def test_ip_attn_folded_every_key_once(hip, case):
    """family A at the four score levels"""
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    assert X.ip_admits(H, keys, ks) and X.ip_sensitivity_a(B // kv_div, H, keys) >= X.IP_MIN_MOVE
    if case == 8:      # the launcher starts at most 256 * 8 / (12 head groups * 4 K/V batches) = 42 workgroups of 64 rows for 43 groups of rows
        assert all(X.ip_grid_x(H, B, S, kv_div, wg)[0] < X.ip_grid_x(H, B, S, kv_div, wg)[1] for wg in range(1, 9))
    want = None
    for level in X.IP_LEVELS:
        sc, v, r = X.ip_family_a(H, keys, B, S, kv_div, level)
        if want is None:                                     # the closed form does not depend on the level
            want, extra = X.ip_expected_a(v, r.to(DEV), kv_div)
        ip_launch(case, f"A ip case {case} c={level:g}", sc, v, r, X.IP_OUT_SCALE_A, lambda got, what: X.check(got, want, what, extra=extra))


@pytest.mark.parametrize("case,out_scale", [(c, 1.0) for c in X.IP_CASES] + [(2, 0.5), (8, 0.5)])
def test_ip_attn_folded_every_row_routed(hip, case, out_scale):
    """family B, bit for bit; out_scale 0.5 (even V codes) at the two shapes with the most paths"""
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    sc, v, r, pi, want = X.ip_family_b(H, keys, B, S, kv_div, out_scale)
    X.ip_check_pi(pi, keys, kv_div, tail_from=2688 if case == 8 else None)
    assert X.ip_leak(torch.softmax(sc.to(DEV).double() * X.IP_SCALE, dim=-1), pi) <= X.IP_LEAK          # on the fp64 reference, before the launch
    want = want.to(DEV)

    def judge(got, what):
        bad = got.double() != want
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[0].tolist()}"
        return 0.0

    ip_launch(case, f"B ip case {case} out_scale={out_scale:g}", sc, v, r, out_scale, judge)


@pytest.mark.parametrize("case", X.IP_G_CASES)
def test_ip_attn_folded_generic(hip, case):
    """family G against the fp64 softmax of the same bf16 inputs"""
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    sc, v, r = X.ip_family_g(H, keys, B, S, kv_div)
    want, mag, _ = X.ip_ref64(sc.to(DEV), v.to(DEV), r.to(DEV), X.IP_SCALE, X.IP_OUT_SCALE_G, kv_div)
    extra = X.ip_tol_g(r.to(DEV), mag)
    ip_launch(case, f"G ip case {case}", sc, v, r, X.IP_OUT_SCALE_G, lambda got, what: X.check(got, want, what, extra=extra))


# ============================================================================================== softmax_rows
def sm_launch(what, x, want, tol):
    """out of place and in place at both row strides -> the worst fraction"""
    from motionrag_amd import ops
    rows, cols = x.shape
    worst = 0.0
    for ld in X.sm_lds(cols):
        for inplace in (False, True):
            b = X.Rows(x, ld, inplace, DEV)
            assert b.x.stride(0) == ld and (b.y.data_ptr() == b.x.data_ptr()) == inplace
            out = ops.softmax_rows(b.x, X.SM_SCALE, out=b.y)
            assert out.data_ptr() == b.y.data_ptr()
            assert b.guards_intact(), f"{what}: an element outside the result was written"
            assert inplace or torch.equal(b.x.float().cpu(), x)
            w = X.check(b.y, want, f"{what} ld={ld}{' in place' if inplace else ''}", **tol)
            print(f"EXACT {what} ld={ld}{' in place' if inplace else ''} {w:.3g}")
            worst = max(worst, w)
    return worst


@pytest.mark.parametrize("cols", X.SM_COLS)
def test_softmax_rows_every_column_once(hip, cols):
    """family C at the three levels"""
    for T in X.SM_LEVELS:
        x = X.sm_family_c(cols, T)
        want = X.sm_ref64(x.to(DEV))
        low = want[x.to(DEV) < T]
        assert low.numel() == 0 or low.max().item() <= 2.0 ** -64             # the leak, on the fp64 reference
        sm_launch(f"C softmax_rows cols={cols} T={T:g}", x, want, X.TOL_SM_C)


@pytest.mark.parametrize("far", [False, True], ids=["48nats", "136nats"])
@pytest.mark.parametrize("cols", X.SM_COLS)
def test_softmax_rows_max_finds_every_column(hip, cols, far):
    """family P: one peak per row, 48 nats above the rest as the sum's and the store's check, 136 nats above as the max's (softmax_exact.py)"""
    x, js = X.sm_family_p(cols, far)
    want = X.sm_ref64(x.to(DEV))
    assert all(want[i, j].item() > 1 - 1e-15 for i, j in enumerate(js))
    sm_launch(f"P softmax_rows cols={cols}{' far' if far else ''}", x, want, X.TOL_SM_C)


@pytest.mark.parametrize("cols", X.SM_COLS)
def test_softmax_rows_generic(hip, cols):
    """family G against the fp64 softmax"""
    x = X.sm_family_g(cols)
    sm_launch(f"G softmax_rows cols={cols}", x, X.sm_ref64(x.to(DEV)), X.TOL_SM_G)
