"""Host-only proof that the exact normalisation tests (test_gpu_norm_exact.py) can fail: no kernel is involved.  For every shape of the GPU tests the two input
families of norm_exact.py are built and judged against fp32 host models of the kernels' statistics forms (two-pass LayerNorm; one-pass GroupNorm from chunk
partials, unsplit and sharded), which must pass, and against the same models with one named mistake ("mutants"), each of which family A must refuse on at
least one shape.  The builder conditions (bf16-exact inputs, integer sums below 2^24, a probe on every 8-vector / chunk edge / remainder pixel, a background
away from zero, no deep cancellation behind the AdaLN shift) are checked beside them.

MUTANT TABLE -- the worst error of the mutant's result as a multiple of the family A bound (2^-8 + 2^-14) |want|, on the shape that kills it best / least
(shapes that give the mistake nothing to act on are left out), and beside it what the N(0, 1) inputs of test_gpu_kernels.test_layernorm (randn * 2 + 0.5, scale 1) and
test_gpu_unet.test_groupnorm (randn * 1.5 + 0.3, SiLU, scale 0.6) make of the same mutant under `close()`: worst error as a multiple of that tolerance.

  LayerNorm (D = 64 ... 8 192)        family A        N(0, 1) under close()
    drop_vec  (8-vector 1)            530 - 1 890     5.5 at D = 64, 1.8 at 320, 0.60 at 1 024, 0.28 at 3 072, 0.20 at 8 192: PASSES from D = 1 024 up
    next_row                          228 - 2 120     3.3 - 12.7 (the neighbour's mean is 2 / sqrt(D) sigma away: seen at small |want| only, 7 % of the elements at 8 192)
    gamma_next_vec                    2 270 - 4 300   15 - 31
  GroupNorm                           family A        N(0, 1) under close()
    drop_last_pixel                   566 - 1 140     0.18 - 0.29 at 600 pixels and more: PASSES (0.91 at 100 pixels, 1.4 at 40)
    drop_chunk_last                   580 - 1 850     0.91 with one chunk (3, 100, 256): PASSES; 1.35 - 1.44 at 18 to 72 chunks, outside on 1 - 3 % of the elements; 33 where a chunk holds two pixels
    drop_remainder                    470 - 490 000   2.5 - 34 000 (with 32 rows per pass and 32-pixel chunks the remainder loop sums everything)
    chunk_twice                       78 - 135        0.68 at 72 chunks: PASSES; 1.4 - 2.4 at 18 to 64 chunks; 20 with one
    stale_empty                       355             14 (only (3, 100, 256) with 64 chunks has empty ones)
    cnt_no_cpg                        91 - 535        19 - 45
    cnt_short                         2.6 - 9.0       0.57 at 72 chunks, 0.81 at 64: PASSES; 1.2 at 31, 2.1 at 18
    segment_drop                      3.0             20 on 2 % of the elements (only C = 2 560 has a straddling group; the spike of group 25 sits in front of 2 048)
    group_next / sample_next          250 - 460       2.6 - 8.9, on 13 - 45 % of the elements
    gamma_next_vec                    2 270 - 4 300   54 - 97
  sharded GroupNorm (256 | 200 | 144 pixels)
    hw_one_shard                      156             28
    shard_missing                     796             8.7

What today's tolerance lets through is therefore the SMALL miscount -- one 8-vector of a wide row, one pixel, one chunk among 64 or more, a count short by one
chunk -- which is what an off-by-one in a clamp, a loop remainder or a chunk plan produces; the gross ones (a wrong gamma vector, a count without cpg) it catches.
Family A refuses every one of them, the smallest by a factor 2.6, and every miscount of single elements by 470 and more."""
import pytest
import torch

import norm_exact as X
from test_gpu_kernels import close

LN_ALL = sorted({(X.ln_rows(D), D) for Ds in X.LN_DIMS.values() for D in Ds} | {(X.LN_ROWS_ROWS, D) for D in X.LN_ROWS_DIMS} | {(131, 1024), (X.ln_rows(512), 512)})
GN_ALL = [(s, X.gn_chunks(s[0], s[1])) for s in X.GN_SHAPES] + [(X.GN_RAW, 64), (X.GN_RAW, 1)]


def ids(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


# ---------------------------------------------------------------------------------------------- the exact models pass
@pytest.mark.parametrize("rows,D", LN_ALL, ids=lambda v: str(v))
def test_layernorm_model_passes_both_families(rows, D):
    x, g = X.ln_family_a(rows, D), X.gamma_pattern(D)
    assert X.bf16_exact(x) and X.bf16_exact(g) and (x * x).sum(-1).max().item() < 2 ** 24
    cols = X.ln_spike_cols(rows, D)
    assert (x[torch.arange(rows), cols].abs() >= X.spike_amp(D)).all() and (x.abs() > 1).sum().item() == rows      # one spike per row, where the map says
    if rows >= D // 8:
        assert set((cols // 8).tolist()) == set(range(D // 8))                                                      # every 8-vector of the row is probed
    assert len(set((cols % 8).tolist())) == min(8, rows)
    assert X.min_background(X.ln_ref64(x)[0]) >= (X.MIN_BACKGROUND if D <= 64 else 0.15)
    for gamma, rms in ((g, False), (None, False), (g, True)):
        want = X.ln_ref64(x, gamma, None, rms=rms)[0]
        assert X.worst_a(X.ln_model(x, gamma, None, rms=rms), want) <= 1.0
        assert X.worst_a(X.bf(want), want) <= 256.0 / 257.0 + 1e-3                                                  # the bound is bf16's own rounding bound, not twice it
    xb, gb, bb = X.ln_family_b(rows, D)
    for gamma, beta in ((gb, bb), (None, None)):
        want, lin, off = X.ln_ref64(xb, gamma, beta)
        assert X.worst_b(X.ln_model(xb, gamma, beta), want, lin, off, X.C_LN) <= 1.0
    # what the third term of the family B bound is there for: the fp32 mean's own rounding on the elements beside the mean
    want, lin, off = X.ln_ref64(xb, gb, bb)
    assert X.worst(X.ln_model(xb, gb, bb), want, X.ULP, extra=X.C_LN * lin + X.C_MEAN * off) <= 1.0


def test_layernorm_stream_shape_model_passes():
    """8 197 rows of 3 072, modulated with the split inside a wave's stride and unmodulated (the GPU case's inputs)"""
    rows, D = X.LN_STREAM
    x, g = X.ln_family_a(rows, D), X.gamma_pattern(D)
    want = X.ln_ref64(x, g)[0]
    assert X.worst_a(X.ln_model(x, g), want) <= 1.0
    assert X.worst_a(X.ln_model(x, g, mutant="drop_vec", arg=383), want) >= 100.0


def test_adaln_case():
    """rows 131 in samples of 65 with the split at 37: shift / scale powers of two; the shift never cancels the normalised term below 2^-6 of it, so the fp32
    rounding of that term (2^-24 of it) stays far inside the bound's 2^-14"""
    rows, D, rpb, split = 131, 1024, 65, 37
    x, g = X.ln_family_a(rows, D), X.gamma_pattern(D)
    mod = X.adaln_pow2(3, D)
    assert X.bf16_exact(mod) and X.bf16_exact(1 + mod[:, 1]) and not torch.equal(mod[0], mod[1]) and not torch.equal(mod[:, 0], mod[:, 2])
    sh, sc = X.adaln_rows(rows, rpb, split, mod)
    assert torch.equal(sh[36], mod[0, 0]) and torch.equal(sh[37], mod[0, 2]) and torch.equal(sh[65], mod[1, 0]) and torch.equal(sc[130], mod[2, 1])
    want, lin, _ = X.ln_ref64(x, g, None, mod=(sh, sc))
    assert (want.abs() / lin).min().item() >= 2.0 ** -6
    assert X.worst_a(X.ln_model(x, g, None, mod=(sh, sc)), want) <= 1.0
    for wrong in (X.adaln_rows(rows, rpb, split + 1, mod), X.adaln_rows(rows, rpb + 1, split, mod)):                # the pair of the neighbouring segment / sample
        assert X.worst_a(X.ln_model(x, g, None, mod=wrong), want) >= 100.0


def test_head_rows_of_the_qk_norm():
    """64-wide head rows with A = 16: the spike amplitude the rule gives, integer sums, eight probed vectors per 8 rows"""
    assert X.spike_amp(64) == 16.0
    x = X.ln_family_a(24, 64)
    assert set((X.ln_spike_cols(24, 64) // 8).tolist()) == set(range(8))
    want = X.ln_ref64(x, X.gamma_pattern(64), eps=1e-6)[0]
    assert X.worst_a(X.ln_model(x, X.gamma_pattern(64), eps=1e-6), want) <= 1.0


@pytest.mark.parametrize("shape,chunks", GN_ALL, ids=ids)
def test_groupnorm_model_passes_both_families(shape, chunks):
    N, HW, C, G = shape
    g, e = X.gamma_pattern(C), X.gn_emb_a(N, C)
    assert X.bf16_exact(e)
    probes = X.gn_probe_pixels(HW, C, chunks)
    ppc = -(-HW // chunks)
    for silu in (False, True):
        x, where = X.gn_family_a(N, HW, C, G, chunks=chunks, silu=silu, gamma=g)
        assert X.bf16_exact(x) and (x.abs() > 1).sum().item() == N * G
        sq = (x * x).view(N, HW, G, C // G).sum((1, 3))
        assert sq.max().item() < 2 ** 24 and (sq > 2.4 * HW * (C // G)).all()                                      # the spike carries 3/5 of the sum of squares or more
        hit = set(where.flatten().tolist())
        assert hit >= set(probes[:N * G]) and HW - 1 in hit and 0 in hit
        if N * G >= len(probes):                                                                                   # enough units: both ends of every chunk
            assert all(k * ppc in hit and min(HW, (k + 1) * ppc) - 1 in hit for k in range(-(-HW // ppc)))
        for emb in (None, e):
            want = X.gn_ref64(x, G, g, None, emb=emb, silu=silu)[0]
            assert X.min_background(X.gn_ref64(x, G, emb=emb)[0]) >= X.MIN_BACKGROUND
            assert X.worst_a(X.gn_model(x, G, chunks, g, None, emb=emb, silu=silu), want) <= 1.0
        xp, _ = X.gn_family_a(N, HW, C, G, chunks=chunks, silu=silu)                                              # no gamma: with SiLU every spike is positive
        assert not silu or (xp.abs() > 1).sum().item() == (xp > 1).sum().item()
        assert X.worst_a(X.gn_model(xp, G, chunks, emb=e, silu=silu), X.gn_ref64(xp, G, emb=e, silu=silu)[0]) <= 1.0
    for emb in (False, True):
        xb, gb, bb, eb = X.gn_family_b(N, HW, C, G, emb=emb)
        for silu in (False, True):
            want, lin, off = X.gn_ref64(xb, G, gb, bb, emb=eb, silu=silu)
            assert X.worst_b(X.gn_model(xb, G, chunks, gb, bb, emb=eb, silu=silu), want, lin, off, X.C_GN) <= 1.0
    # mu / sigma = 128: what the one-pass variance keeps of rstd in this model's summation order (the kernels' own figure is in DESIGN.md)
    xb, gb, bb, _ = X.gn_family_b(N, HW, C, G, ratio=128)
    gs, gq = X.gn_group_sums(xb, G, chunks)
    rho = (X.rstd_fp32(gs, gq, HW * (C // G)).double() / X.rstd_ref64(xb, G) - 1).abs().max().item()
    print(f"NORM-EXACT model rstd error at mu / sigma = 128 {shape} chunks {chunks}: {rho:.3g}")
    assert rho < 2.0 ** -8


def test_sharded_groupnorm_model_passes():
    N, sizes, C, G = X.GN_SPLIT
    g, HW = X.gamma_pattern(C), sum(X.GN_SPLIT[1])
    x, where = X.gn_family_a(N, HW, C, G, pixels=X.split_probe_pixels(sizes, C, N))
    edges = [0, sizes[0], sizes[0] + sizes[1], HW]
    for i in range(3):                                                                                             # probes in every shard, on its first and last pixel
        assert {edges[i], edges[i + 1] - 1} <= set(where.flatten().tolist())
    shards = list(torch.split(x, list(sizes), dim=1))
    want = X.gn_ref64(x, G, g)[0]
    assert X.worst_a(X.gn_split_model(shards, G, g), want) <= 1.0
    xb, gb, bb, _ = X.gn_family_b(N, HW, C, G)
    wb, lin, off = X.gn_ref64(xb, G, gb, bb)
    assert X.worst_b(X.gn_split_model(list(torch.split(xb, list(sizes), dim=1)), G, gb, bb), wb, lin, off, X.C_GN) <= 1.0


@pytest.mark.parametrize("case", X.GN_MOD, ids=lambda c: ids(c[1]) + f"-C{c[2]}")
def test_mod_form_model_passes(case):
    N, (T, H, W), C, shift, split, Tz = case
    HW, G = T * H * W, 32
    mod = X.mod_maps(N, Tz, H >> shift, W >> shift, C)
    assert X.bf16_exact(mod) and (mod[..., C:] == 0).all() and len(torch.unique(mod[..., 0])) >= 4
    sc, sh = X.mod_full(mod, T, H, W, shift, split)
    assert sc.shape == (N, HW, C) and torch.equal(sc[:, 0], mod[:, 0, 0, 0, :C]) and torch.equal(sc[:, -1], mod[:, -1, -1, -1, :C])
    if split:                                                                                                      # frame 0 alone from latent frame 0
        assert torch.equal(sc[:, H * W - 1], mod[:, 0, -1, -1, :C]) and torch.equal(sc[:, H * W], mod[:, 1, 0, 0, :C])
    g = X.gamma_pattern(C)
    x, _ = X.gn_family_a(N, HW, C, G)
    want = X.gn_ref64(x, G, g, None, mod=(sc, sh))[0]
    assert X.worst_a(X.gn_model(x, G, X.gn_chunks(N, HW), g, None, mod=(sc, sh)), want) <= 1.0
    wrong = X.mod_full(mod.roll(1, 3), T, H, W, shift, split)                                                       # the map of the latent pixel to the left
    assert X.worst_a(X.gn_model(x, G, X.gn_chunks(N, HW), g, None, mod=wrong), want) >= 100.0
    mb = X.mod_maps(N, Tz, H >> shift, W >> shift, C, family="B")
    xb, gb, bb, _ = X.gn_family_b(N, HW, C, G)
    scb, shb = X.mod_full(mb, T, H, W, shift, split)
    wb, lin, off = X.gn_ref64(xb, G, gb, bb, silu=True, mod=(scb, shb))
    assert X.worst_b(X.gn_model(xb, G, X.gn_chunks(N, HW), gb, bb, silu=True, mod=(scb, shb)), wb, lin, off, X.C_GN) <= 1.0


# ---------------------------------------------------------------------------------------------- every mutant fails family A
def _n01_ln(rows, D):
    g = torch.Generator().manual_seed(rows)
    return (X.bf(torch.randn(rows, D, generator=g) * 2 + 0.5).float(), X.bf(1 + 0.1 * torch.randn(D, generator=g)).float(), X.bf(0.1 * torch.randn(D, generator=g)).float())


def _n01_gn(N, HW, C):
    g = torch.Generator().manual_seed(1)
    return (X.bf(torch.randn(N, HW, C, generator=g) * 1.5 + 0.3).float(), X.bf(1 + 0.2 * torch.randn(C, generator=g)).float(), X.bf(0.2 * torch.randn(C, generator=g)).float())


def _close_share(got, want, scale):
    return ((got.double() - want).abs() / (2e-2 * want.abs() + 2e-2 * scale)).max().item()


@pytest.mark.parametrize("mutant", X.LN_MUTANTS)
def test_layernorm_mutants_fail_family_a(mutant):
    """the module docstring's LayerNorm rows"""
    for D in (64, 320, 1024, 3072, 8192):
        rows, g = X.ln_rows(D), X.gamma_pattern(D)
        x = X.ln_family_a(rows, D)
        want = X.ln_ref64(x, g)[0]
        w = X.worst_a(X.ln_model(x, g, mutant=mutant, arg=1), want)
        xn, wn, bn = _n01_ln(rows, D)
        today = _close_share(X.ln_model(xn, wn, bn, mutant=mutant, arg=1), X.ln_ref64(xn, wn, bn)[0], 1.0)
        print(f"NORM-EXACT mutant {mutant} D={D}: family A {w:.4g} bounds; N(0, 1) under close() {today:.3g}")
        assert w >= 200.0, (mutant, D, w)
        if mutant == "drop_vec":
            # every vector left out is refused on the rows that probe it, by the unit's every element
            j = D // 8 - 1
            got = X.ln_model(x, g, mutant=mutant, arg=j)
            bad = ((got.double() - want).abs() > X.REL_A * want.abs())
            assert bad[torch.arange(rows) % (D // 8) == j].double().mean().item() >= 0.99
            if D >= 1024:                                                                                           # the gap: today's data and tolerance pass it
                close(X.ln_model(xn, wn, bn, mutant=mutant, arg=1), X.ln_ref64(xn, wn, bn)[0], scale=1.0)
                assert today < 0.7


PASSES_TODAY = {("drop_last_pixel", (4, 600, 320, 32), 18), ("drop_last_pixel", (2, 2304, 64, 32), 72), ("drop_last_pixel", (5, 1000, 64, 32), 31),
                ("drop_chunk_last", X.GN_RAW, 1), ("chunk_twice", (2, 2304, 64, 32), 72), ("cnt_short", (2, 2304, 64, 32), 72), ("cnt_short", X.GN_RAW, 64)}
KILL_FLOOR = {"cnt_short": 2.0, "segment_drop": 2.0}


@pytest.mark.parametrize("mutant", X.GN_MUTANTS)
def test_groupnorm_mutants_fail_family_a(mutant):
    """the module docstring's GroupNorm rows: refused on every shape that gives the mistake something to act on, and on at least one"""
    ran = 0
    for shape, chunks in GN_ALL:
        N, HW, C, G = shape
        g = X.gamma_pattern(C)
        x, _ = X.gn_family_a(N, HW, C, G, chunks=chunks)
        got = X.gn_model(x, G, chunks, g, None, mutant=mutant)
        if got is None:
            continue
        ran += 1
        w = X.worst_a(got, X.gn_ref64(x, G, g)[0])
        xn, wn, bn = _n01_gn(N, HW, C)
        ref = X.gn_ref64(xn, G, wn, bn, silu=True)[0]
        today = _close_share(X.gn_model(xn, G, chunks, wn, bn, silu=True, mutant=mutant), ref, 0.6)
        print(f"NORM-EXACT mutant {mutant} {shape} chunks {chunks}: family A {w:.4g} bounds; N(0, 1) under close() {today:.3g}")
        assert w >= KILL_FLOOR.get(mutant, 50.0), (mutant, shape, w)
        if (mutant, shape, chunks) in PASSES_TODAY:
            close(X.gn_model(xn, G, chunks, wn, bn, silu=True, mutant=mutant), ref, scale=0.6)
    assert ran >= 1


@pytest.mark.parametrize("mutant", X.SPLIT_MUTANTS)
def test_sharded_mutants_fail_family_a(mutant):
    N, sizes, C, G = X.GN_SPLIT
    g, HW = X.gamma_pattern(C), sum(sizes)
    x, _ = X.gn_family_a(N, HW, C, G, pixels=X.split_probe_pixels(sizes, C, N))
    w = X.worst_a(X.gn_split_model(list(torch.split(x, list(sizes), dim=1)), G, g, mutant=mutant), X.gn_ref64(x, G, g)[0])
    print(f"NORM-EXACT mutant {mutant}: family A {w:.4g} bounds")
    assert w >= 100.0


def test_comparator():
    want = torch.tensor([[0.5, -2.0, 0.0]], dtype=torch.float64)
    assert X.worst_a(want.clone(), want) == 0.0
    assert X.worst_a(torch.tensor([[0.5 * (1 + 2.0 ** -9), -2.0, 0.0]]), want) == pytest.approx(0.5 / (1 + 2.0 ** -6), rel=1e-6)
    assert X.worst_a(torch.tensor([[0.5, -2.0, 1e-30]]), want) == float("inf")                                      # a zero bound is met exactly or not at all
    assert X.worst_b(torch.tensor([[0.5, -2.0, 1e-6]]), want, torch.full((1, 3), 2.0 ** -9), torch.zeros(1, 3), X.C_GN) == pytest.approx(1e-6 * 2 ** 18)
    with pytest.raises(AssertionError):
        X.worst_a(torch.tensor([[float("nan"), -2.0, 0.0]]), want)
    with pytest.raises(AssertionError):
        X.check(1.01, "x")
    assert X.gn_chunks(4, 600) == 18 and X.gn_chunks(2, 2304) == 72 and X.gn_chunks(1, 40) == 1 and X.gn_chunks(5, 1000) == 31
    assert X.gn_rpps(320) == [6] and X.gn_rpps(2560) == [1, 4] and X.gn_rpps(64) == [32]
