"""Host-only proof that the exact softmax tests (test_gpu_softmax_exact.py) can fail and that a correct kernel passes them: no kernel is involved.  For every
shape the GPU file uses, the builder conditions of softmax_exact.py are evaluated (bf16-exact inputs, the 4-bound sensitivity, the leak, the V code, the keys a
map must hit, the launcher's grid at case 8); the checks must accept the fp64 reference and an fp32 emulation of the kernel's rounding points, and refuse every
fp64 "mutant" -- a restatement of the kernel with one fault -- that the family is not blind to by design (IP_BLIND / SM_BLIND and the module docstring there)."""
import pytest
import torch

import softmax_exact as X

SMALL_IP = [c for c in X.IP_CASES if c != 8]


def refuses_exactly(got, want):
    return not torch.equal(got, want)


# ============================================================================================== ip_attn_folded
@pytest.mark.parametrize("case", list(X.IP_CASES))
def test_ip_shapes_are_admitted_and_sensitive(case):
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    assert X.ip_admits(H, keys, ks) and B % kv_div == 0
    assert X.ip_min_width(H, ks, "ops") >= X.ip_min_width(H, ks, "c") >= (H - 1) * ks + keys
    assert X.ip_sensitivity_a(B // kv_div, H, keys) >= X.IP_MIN_MOVE
    pi = X.ip_pi(H, keys, B, S, kv_div)
    X.ip_check_pi(pi, keys, kv_div, tail_from=2688 if case == 8 else None)
    assert B * H == 1 or not all(torch.equal(pi[0, :, 0], pi[b, :, h]) for b in range(B) for h in range(H))
    for even in (False, True):
        X.ip_check_code(X.ip_v_code(B // kv_div, H, keys, even))
    # the leak, on the fp64 softmax of family B's scores
    sc = X.ip_family_b(H, keys, B, S, kv_div)[0]
    assert X.ip_leak(torch.softmax(sc.double() * X.IP_SCALE, dim=-1), pi) <= X.IP_LEAK


def test_ip_case_3_shift_7_and_case_8_second_trip():
    H, keys, ks = X.IP_CASES[3][:3]
    assert sorted((ks * h) & 7 for h in range(H))[-1] == 7 and X.ip_admits(H, keys, ks) and not X.ip_admits(H, keys + 1, ks + 2)    # (27 h) & 7 reaches 7 too
    assert sorted({(X.IP_CASES[2][2] * h) & 7 for h in range(3)}) == [0, 2, 4]
    H, keys, ks, B, S, kv_div = X.IP_CASES[8]
    for wg in range(1, 9):                 # a workgroup of four waves puts one wave on each SIMD, eight waves per SIMD: at most 8 workgroups per CU
        gx, groups = X.ip_grid_x(H, B, S, kv_div, wg)
        assert gx < groups == 43 and gx <= 42
    assert 42 * 64 == 2688 < S


@pytest.mark.parametrize("case", SMALL_IP)
def test_ip_family_a_reference_emulation_and_mutants(case):
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    os_ = X.IP_OUT_SCALE_A
    for level in X.IP_LEVELS:
        sc, v, r = X.ip_family_a(H, keys, B, S, kv_div, level)
        want, extra = X.ip_expected_a(v, r, kv_div)
        ref = X.ip_ref64(sc, v, r, X.IP_SCALE, os_, kv_div)[0]
        assert (ref - want).abs().max().item() < 1e-13                            # the closed form IS the fp64 softmax of these inputs
        assert X.passes(X.rbf(want), want, extra=extra)
        assert X.passes(X.ip_emulate32(sc, v, r, X.IP_SCALE, os_, kv_div), want, extra=extra)
        ran = 0
        for kind in X.IP_MUTANTS:
            if kind == "pad_zero" and level == 384.0:
                continue                                                          # a slot at score 0 is 48 nats under this level
            m = X.ip_mutant(kind, sc, v, r, X.IP_SCALE, os_, kv_div)
            if m is None or (keys == 1 and kind in ("dup_first", "next_key")):    # one key: doubled it is still the whole softmax
                continue
            assert X.worst(X.rbf(X.f32(m)), want, extra=extra) >= X.IP_MIN_MOVE, (kind, level)
            ran += 1
        assert ran >= (3 if keys == 1 else 6), ran


@pytest.mark.parametrize("case", SMALL_IP)
def test_ip_family_b_reference_emulation_and_mutants(case):
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    for out_scale, fam in ((1.0, "B1"), (0.5, "B")):
        sc, v, r, pi, want = X.ip_family_b(H, keys, B, S, kv_div, out_scale)
        ref, _, p = X.ip_ref64(sc, v, r, X.IP_SCALE, out_scale, kv_div)
        assert X.ip_leak(p, pi) <= X.IP_LEAK and (ref - want).abs().max().item() <= 2.0 ** -50      # (where r + V cancels, the leak is what is left)
        assert torch.equal(X.ip_emulate32(sc, v, r, X.IP_SCALE, out_scale, kv_div), want)
        ran = 0
        for kind in X.IP_MUTANTS:
            m = X.ip_mutant(kind, sc, v, r, X.IP_SCALE, out_scale, kv_div)
            if m is None or kind in X.IP_BLIND[fam]:
                continue
            assert refuses_exactly(X.rbf(X.f32(m)), want), (kind, fam)
            ran += 1
        assert ran >= (2 if keys == 1 else 5), ran


@pytest.mark.parametrize("case", X.IP_G_CASES + (5, 9))
def test_ip_family_g_reference_emulation_and_mutants(case):
    """cases 5 and 9 are the issue's other two emulation shapes, (32, 4) and (9, 3)"""
    H, keys, ks, B, S, kv_div = X.IP_CASES[case]
    os_ = X.IP_OUT_SCALE_G
    sc, v, r = X.ip_family_g(H, keys, B, S, kv_div)
    want, mag, _ = X.ip_ref64(sc, v, r, X.IP_SCALE, os_, kv_div)
    extra = X.ip_tol_g(r, mag)
    assert X.passes(X.rbf(X.f32(want)), want, extra=extra)
    w = X.worst(X.ip_emulate32(sc, v, r, X.IP_SCALE, os_, kv_div), want, extra=extra)
    print(f"emulation G case {case}: {w:.3g} of the bound")
    assert w <= 1.0
    for kind in X.IP_MUTANTS:
        m = X.ip_mutant(kind, sc, v, r, X.IP_SCALE, os_, kv_div)
        if m is not None:
            assert X.rejects(X.rbf(X.f32(m)), want, extra=extra), kind


def test_ip_buffers():
    H, keys, ks, B, S, kv_div = X.IP_CASES[2]
    sc, v, r = X.ip_family_a(H, keys, B, S, kv_div, 384.0)
    for W in (X.ip_min_width(H, ks, "c"), X.ip_min_width(H, ks, "ops") + 64):
        buf = X.ip_scores_buffer(sc, ks, W)
        assert buf.shape == (B, S, W) and int(torch.isfinite(buf.float()).sum()) == sc.numel()
        assert all(torch.equal(buf[:, :, ks * h:ks * h + keys].float(), sc[:, :, h]) for h in range(H))
    vb = X.ip_v_buffer(v, "cpu")
    assert torch.equal(vb.float(), v.reshape(B // kv_div, keys, H * 64)) and vb.stride(1) == H * 64 + 16 and vb.storage_offset() % 8 == 0
    for pad in (0, 64):
        hb = X.Hidden(r, "cpu", col_pad=pad)
        assert torch.equal(hb.result().float(), r) and hb.guards_intact() and (pad == 0) == (hb.view is not None)
        hb.inner.fill_(1.0)
        assert hb.guards_intact()
        hb.buf[X.GUARD_ROWS - 1, 0] = 0.0
        assert not hb.guards_intact()
    hb = X.Hidden(r, "cpu", col_pad=64)
    hb.rows[3, H * 64] = 0.0
    assert not hb.guards_intact()


# ============================================================================================== softmax_rows
def sm_cases(cols):
    """(family, label, x, tolerance) of everything the GPU file launches at this row length"""
    out = [("C", f"C T={T:g}", X.sm_family_c(cols, T), X.TOL_SM_C) for T in X.SM_LEVELS]
    out.append(("P", "P", X.sm_family_p(cols)[0], X.TOL_SM_C))
    out.append(("Pfar", "P far", X.sm_family_p(cols, far=True)[0], X.TOL_SM_C))
    out.append(("G", "G", X.sm_family_g(cols), X.TOL_SM_G))
    return out


@pytest.mark.parametrize("cols", X.SM_COLS)
def test_sm_reference_emulation_and_mutants(cols):
    seen = set()
    for fam, label, x, tol in sm_cases(cols):
        want = X.sm_ref64(x)
        assert X.passes(X.rbf(X.f32(want)), want, **tol)
        w = X.worst(X.sm_emulate32(x), want, **tol)
        print(f"emulation {label} cols={cols}: {w:.3g} of the bound")
        # family C sits at half its bound and no lower: bf16(1/24) itself is 0.4995 x 2^-8 off 1/24 (1/24 = 1.333 x 2^-5, 170.67 -> 171 of 128ths)
        assert w <= (0.51 if fam == "C" else 1.0)
        if fam in ("P", "Pfar"):
            js = X.sm_family_p(cols)[1]
            assert all(want[i, j] > 1 - 1e-15 for i, j in enumerate(js))
            assert set(range(cols - cols % 8, cols)) <= set(js) and {0, cols - 1} <= set(js)
        if fam == "C":
            low = want[x < x.amax()]
            assert low.numel() == 0 or low.max().item() <= 2.0 ** -64             # the asserted leak
        for prev in (torch.full_like(x, X.SENTINEL), x):                          # out of place / in place
            for kind in X.SM_MUTANTS:
                m = X.sm_mutant(kind, x, prev)
                if m is None or kind in X.SM_BLIND[fam]:
                    continue
                assert X.rejects(X.rbf(X.f32(m)), want, **tol), (kind, label)
                seen.add(kind)
    expect = {"dup_col0", "no_scale"} if cols > 1 else {"dup_col0"}
    if cols % 8:
        expect |= {"tail_unsummed", "tail_unwritten"}
        if cols > 8:
            expect.add("max_body_only")
    if cols > 512:
        expect.add("max_first_wave")
    assert seen == expect, (seen, expect)


def test_sm_shift_invariance_is_why_far_rows_exist():
    """at the 48-nat gap a max that misses the peak still gives the right row (fp32 holds 2^69); at 136 nats it cannot"""
    x, js = X.sm_family_p(2052)
    i = js.index(2051)
    assert X.passes(X.sm_mutant("max_body_only", x, x)[i:i + 1], X.sm_ref64(x)[i:i + 1], **X.TOL_SM_C)
    xf, _ = X.sm_family_p(2052, far=True)
    assert not torch.isfinite(X.sm_mutant("max_body_only", xf, xf)[i]).all()


def test_sm_buffers():
    x = X.sm_family_g(100)
    assert X.sm_lds(100) == (104, 112) and X.sm_lds(96) == (96, 104)
    for inplace in (False, True):
        b = X.Rows(x, 112, inplace, "cpu")
        assert torch.equal(b.x.float(), x) and b.guards_intact() and (b.y.data_ptr() == b.x.data_ptr()) == inplace
        assert inplace or not torch.isfinite(b.xbuf[:, 100:].float()).any()
        b.y.fill_(0.5)
        assert b.guards_intact()
        b.ybuf[1, 100] = 0.0
        assert not b.guards_intact()
