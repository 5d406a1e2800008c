"""Value tests of the HBM-bound streaming kernels PAST their grid caps: every kernel of pointwise.hip, unet_ops.hip, norm.hip's qknorm_rope_kernel and
preprocess.hip's assemble_tokens_kernel launches at most `cap` workgroups of 256 threads and walks the rest of its work in a grid-stride loop, several of them
carrying (row, column, table row) indices across the stride incrementally.  The shapes here are the smallest that run that stride with a ragged remainder --
one "sweep" is cap x 256 work items -- and every element is compared with a plain fp32 / fp64 torch restatement of the operation on the host.

Tolerances (derived from the number formats, none measured):
  data movement                       torch.equal
  one fp32 expression, one RNE store  |got - exact| <= 2^-8 |exact| + 2^-20 m     exact = the fp64 value, m = the sum of the magnitudes of the terms entering the
                                      element: half a bf16 ulp is at most 2^-8 relative, and the second term (16 fp32 ulps of m) covers the fp32 rounding of the
                                      handful of intermediates, cancellation included
  approximated transcendentals /      test_gpu_kernels.close at its default 2 % + 2 % of the reference's mean magnitude (the bound of the small-shape tests)
  statistics
  ddim_v_step_ (fp32 in and out)      |got - fp64| <= 2^-20 m
Where a kernel rounds an INTERMEDIATE to bf16 by contract (cfg_dpm_step_'s x0, blend_tile's vertical blend in the corner), the restatement rounds there too.  The
fp32 intermediate and the fp64 one may sit on two sides of a bf16 rounding boundary (about one element in 2^10 does at these magnitudes), so every bf16 value
in [bf16(i - s), bf16(i + s)], s = 2^-20 m the fp32 slack of the fp64 intermediate i, is taken as that rounding (rounding is monotone: the kernel's lies there),
and what follows is checked from there with the bound above: no bound is widened."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import bf, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SWEEP_2048 = 2048 * 256            # pointwise.hip: 16-byte vectors (or work items) per sweep
SWEEP_4096 = 4096 * 256            # unet_ops.hip
HALF_ULP, FP32_SLACK = 2.0 ** -8, 2.0 ** -20


def f32(v):
    """the value a C-ABI `float` argument holds"""
    return float(np.float32(v))


def within(got, exact, m, rel=HALF_ULP):
    """elementwise |got - exact| <= rel |exact| + 2^-20 m  ->  (bool tensor, error / bound)"""
    err = (got.cpu().double() - exact).abs()
    tol = rel * exact.abs() + FP32_SLACK * m
    return err <= tol, err / tol.clamp_min(1e-300)


def bounded(name, got, exact, m, rel=HALF_ULP, sweep=None, ok=None):
    """assert the bound on every element; a failure names the first and last offending flat index and, given the sweep length in elements, their sweeps"""
    assert tuple(got.shape) == tuple(exact.shape), (got.shape, exact.shape)
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    if ok is None:
        ok, ratio = within(got, exact, m, rel)
        print(f"{name}: worst element at {ratio.max().item():.3f} x the bound")
    if not bool(ok.all()):
        bad = (~ok).flatten().nonzero().flatten()
        where = f"first flat index {bad[0].item()}, last {bad[-1].item()}"
        if sweep:
            where += f" (sweeps {bad[0].item() // sweep} .. {bad[-1].item() // sweep} of {sweep} elements)"
        raise AssertionError(f"{name}: {bad.numel()} / {ok.numel()} elements outside the bound; {where}")


def refused(fn):
    """`fn` must raise from the wrapper (ValueError) or from the C ABI's argument check (MRAG_EINVAL) -- not from a launch"""
    from motionrag_amd._lib import HipError
    with pytest.raises((ValueError, HipError)) as e:
        fn()
    assert isinstance(e.value, ValueError) or "MRAG_EINVAL" in str(e.value), e.value


def randbf(g, *shape, scale=1.0, shift=0.0):
    return bf(torch.randn(*shape, generator=g) * scale + shift)


# ---------------------------------------------------------------------------------------------- cap 2 048 workgroups (pointwise.hip)
N_TAIL = 2 * 8 * SWEEP_2048 + 2400 + 5      # 1 048 876 vectors: two sweeps of 524 288, a partial third of 300, and a scalar tail of 5 elements
N_EVEN = 2 * 8 * SWEEP_2048 + 2400          # the same without the scalar tail (these kernels take n % 8 == 0 only)


@pytest.mark.parametrize("n", [N_TAIL, 5, 8, 13])
def test_silu_add_past_the_grid_cap(hip, n):
    """silu_kernel / add_kernel, cap 2 048 workgroups = 524 288 vectors per sweep.  n = 8 393 605: 1 048 876 vectors = two full sweeps + 300 vectors of a third
    + 5 scalar-tail elements (workgroup 0).  The degenerate ends: n = 5 (no vector at all: a one-workgroup grid that only runs the tail), 8 (one vector, no
    tail), 13 (one vector + tail).  silu: `close` (v_exp / v_rcp approximations); add: one exact fp32 sum, one rounding."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(100 + n % 97)
    x, y = randbf(g, n, scale=3.0), randbf(g, n, scale=3.0)
    got = ops.silu(x.to(DEV))
    assert got.shape == x.shape
    close(got, F.silu(x.float()))
    bounded(f"add n={n}", ops.add(x.to(DEV), y.to(DEV)), x.double() + y.double(), x.double().abs() + y.double().abs(), sweep=8 * SWEEP_2048)


def test_axpby_past_the_grid_cap(hip):
    """axpby_kernel, cap 2 048 workgroups: n = 8 391 008 = 1 048 876 vectors = two sweeps of 524 288 + 300 vectors"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(111)
    x, y = randbf(g, N_EVEN, scale=2.0), randbf(g, N_EVEN, scale=2.0)
    a, b = f32(0.3), f32(-1.7)
    got = ops.axpby(x.to(DEV), y.to(DEV), a, b)
    bounded("axpby", got, a * x.double() + b * y.double(), (a * x.double()).abs() + (b * y.double()).abs(), sweep=8 * SWEEP_2048)


def _cfg_inputs(seed, n):
    g = torch.Generator().manual_seed(seed)
    v, x = randbf(g, 2, n), randbf(g, n, scale=1.5)
    return g, v, x, v[0].double(), v[1].double(), x.double()


def test_cfg_ddim_step_past_the_grid_cap(hip):
    """cfg_ddim_kernel, cap 2 048 workgroups: n = 8 391 008 = two sweeps of 524 288 vectors + 300 (the conditional half is read at offset n)"""
    from motionrag_amd import ops
    _, v, x, vu, vc, xx = _cfg_inputs(112, N_EVEN)
    gd, sa, sb, a, b = f32(6.0), f32(0.83), f32(0.56), f32(0.61), f32(0.37)
    got = ops.cfg_ddim_step_(v.to(DEV), x.to(DEV).clone(), gd, sa, sb, a, b)
    vv, mv = vu + gd * (vc - vu), vu.abs() + gd * (vc.abs() + vu.abs())
    exact = a * xx + b * (sa * xx - sb * vv)
    m = (a * xx).abs() + b * ((sa * xx).abs() + sb * mv)
    bounded("cfg_ddim_step_", got, exact, m, sweep=8 * SWEEP_2048)


@pytest.mark.parametrize("second_order", [False, True])
def test_cfg_dpm_step_past_the_grid_cap(hip, second_order):
    """cfg_dpm_kernel, cap 2 048 workgroups: n = 8 391 008 = two sweeps of 524 288 vectors + 300.  x0 = bf16(sa x - sb v) is rounded by contract (the
    reference carries it between steps in the latents' dtype): the updated `x0_prev` must be a bf16 rounding of a value within the fp32 slack of the fp64 x0,
    i.e. lie in [bf16(x0 - slack), bf16(x0 + slack)] -- one value, or two neighbours at a rounding boundary, or a few more where x0 cancels (module
    docstring) -- and the new latents are checked with the one-rounding bound from the x0 the kernel stored."""
    from motionrag_amd import ops
    g, v, x, vu, vc, xx = _cfg_inputs(113 + second_order, N_EVEN)
    x0_old, noise = randbf(g, N_EVEN), randbf(g, N_EVEN)
    gd, sa, sb, m1, m2, m3, m4, mn = (f32(c) for c in (6.0, 0.83, 0.56, 0.93, -0.41, 1.45, 0.45, 0.21))
    xd, x0d = x.to(DEV).clone(), x0_old.to(DEV).clone()
    got = ops.cfg_dpm_step_(v.to(DEV), xd, x0d, noise.to(DEV), gd, sa, sb, m1, m2, m3, m4, mn, second_order)
    vv, mv = vu + gd * (vc - vu), vu.abs() + gd * (vc.abs() + vu.abs())
    x0 = sa * xx - sb * vv
    slack = FP32_SLACK * ((sa * xx).abs() + sb * mv)
    x0_got = x0d.cpu()
    is_rounding = (x0_got.double() >= bf(x0 - slack).double()) & (x0_got.double() <= bf(x0 + slack).double())          # rounding is monotone
    bounded("cfg_dpm_step_ x0_prev", x0_got, x0, slack, sweep=8 * SWEEP_2048, ok=is_rounding)
    x0u, xo = x0_got.double(), x0_old.double()
    d, md = (m3 * x0u - m4 * xo, (m3 * x0u).abs() + (m4 * xo).abs()) if second_order else (x0u, x0u.abs())
    exact = m1 * xx - m2 * d + mn * noise.double()
    m = (m1 * xx).abs() + abs(m2) * md + (mn * noise.double()).abs()
    bounded(f"cfg_dpm_step_ second_order={second_order}", got, exact, m, sweep=8 * SWEEP_2048)


def test_add_rows_past_the_grid_cap(hip):
    """add_rows_kernel, cap 2 048 workgroups: x [3, 2500, 640] = 600 000 vectors = one sweep of 524 288 + 75 712; the table's period (2 500 rows = 200 000
    vectors) does not divide the stride, so the second sweep meets every thread at another table row than the first"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(114)
    x, tab = randbf(g, 3, 2500, 640), randbf(g, 2500, 640)
    got = ops.add_rows(x.to(DEV), tab.to(DEV))
    bounded("add_rows", got, x.double() + tab.double()[None], x.double().abs() + tab.double().abs()[None], sweep=8 * SWEEP_2048)


ADD_BCAST = [(20000, 320, 72, 14, False),       # 800 000 vectors: 1 sweep + 275 712; stride = 13 107 rows + 8 of 40 columns: the column index carries into the row
             (9000, 960, 7, 3, False),          # 1 080 000 vectors: 2 sweeps + 31 424; D / 8 = 120 is no power of two (stride = 4 369 rows + 8 columns)
             (70000, 64, 1, 5, False),          # 560 000 vectors: 1 sweep + 35 712; div = 1: the group changes -- and the kernel divides -- every step
             (5000, 1280, 5000, 2, False),      # 800 000 vectors: 1 sweep + 275 712; div (5 000 rows) larger than the stride in rows (3 276): mostly no crossing
             (40000, 320, 1152, 3, False),      # 1 600 000 vectors: 3 sweeps + 27 136; the stride (13 107 rows) crosses eleven groups of 1 152 rows at a time
             (20000, 320, 72, 14, True)]        # the first case with `table` a column slice of a wider matrix (row stride 344 > D = 320 elements)


@pytest.mark.parametrize("rows,D,div,period,sliced", ADD_BCAST)
def test_add_bcast_past_the_grid_cap(hip, rows, D, div, period, sliced):
    """add_bcast_kernel, cap 2 048 workgroups = 524 288 vectors per sweep: (row, column vector, table row, offset in the group) advance by (rstep, cstep) with a
    carry per grid stride and divide only when a group of `div` rows is crossed.  Sweeps and tails per case: see ADD_BCAST."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(rows + div)
    x, wide = randbf(g, rows, D), randbf(g, period, D + 24)
    tab = wide[:, 8:8 + D]
    tab_dev = wide.to(DEV)[:, 8:8 + D] if sliced else tab.contiguous().to(DEV)
    assert (tab_dev.stride(0) == D + 24) == sliced
    got = ops.add_bcast(x.to(DEV), tab_dev, div)
    t = tab.double()[(torch.arange(rows) // div) % period]
    bounded(f"add_bcast {rows}x{D} div {div} period {period}", got, x.double() + t, x.double().abs() + t.abs(), sweep=8 * SWEEP_2048)


def test_cfg_euler_step_past_the_grid_cap(hip):
    """cfg_euler_kernel, cap 2 048 workgroups: latents [3, 14, 4, 144, 256] = 774 144 vectors = one sweep of 524 288 + 249 856, a frame = 18 432 vectors.  With
    a per-frame guidance ramp the frame index (recomputed per iteration, modulo F) wraps from sample 1 to sample 2 inside the second sweep."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(115)
    shape = (3, 14, 4, 144, 256)
    v, x = randbf(g, 2, *shape), randbf(g, *shape, scale=4.0)
    gs = torch.linspace(1.0, 3.0, 14)
    cx, cv = f32(0.93), f32(-0.41)
    got = ops.cfg_euler_step_(v.to(DEV), x.to(DEV).clone(), gs.to(DEV), cx, cv)
    vu, vc, xx, gg = v[0].double(), v[1].double(), x.double(), gs.double().view(1, 14, 1, 1, 1)
    exact = cx * xx + cv * (vu + gg * (vc - vu))
    m = (cx * xx).abs() + abs(cv) * (vu.abs() + gg * (vc.abs() + vu.abs()))
    bounded("cfg_euler_step_", got, exact, m, sweep=8 * SWEEP_2048)


@pytest.mark.parametrize("shape", [(2, 3, 525, 8200), (4, 9, 40)])
def test_weighted_sum(hip, shape):
    """weighted_sum_kernel, cap 2 048 workgroups per sample (grid.y = sample): x [2, 3, 525, 8200] has n / 8 = 538 125 vectors per sample = one sweep of
    524 288 + 13 837; [4, 9, 40] is five vectors (K = 9: the 'mean' fusion's width).  fp32 weights and `w=None` with div = 3 / 9 (the mean); fp32 fmaf
    accumulation in k order, one division, one rounding -> the one-rounding bound against the fp64 sum."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    B, K = shape[:2]
    x = randbf(g, *shape, scale=2.0)
    w = torch.randn(B, K, generator=g)
    xd = x.to(DEV)
    for wt, div in ((w, 1.0), (None, float(K))):
        got = ops.weighted_sum(xd, None if wt is None else wt.to(DEV), div)
        assert got.shape == (B, *shape[2:])
        ww = (torch.ones(B, K) if wt is None else wt).double().view(B, K, *([1] * (len(shape) - 2)))
        exact, m = torch.zeros(B, *shape[2:], dtype=torch.float64), torch.zeros(B, *shape[2:], dtype=torch.float64)
        for k in range(K):
            term = ww[:, k] * x[:, k].double()
            exact += term
            m += term.abs()
        bounded(f"weighted_sum {shape} w={'none' if wt is None else 'fp32'} div={div}", got, exact / div, m / div)


def test_patchify_unpatchify_past_the_grid_cap(hip):
    """patchify_kernel / unpatchify_kernel, cap 2 048 workgroups = 524 288 work items per sweep: B = 2 (both reading latent 0: Bl = 1), F = 5, C0 = C1 = 16,
    96 x 144 -> 2 * 5 * 48 * 72 * 32 = 1 105 920 items = two sweeps + 57 344.  Bit-exact both ways."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(116)
    B, Bl, Fr, C, H, W = 2, 1, 5, 16, 96, 144
    lat, img = randbf(g, Bl, Fr, C, H, W), randbf(g, Bl, Fr, C, H, W)
    rows = ops.patchify(lat.to(DEV), img.to(DEV), B)
    x = torch.cat([lat, img], dim=2).repeat(B, 1, 1, 1, 1).float()
    want = F.unfold(x.reshape(B * Fr, 2 * C, H, W), kernel_size=2, stride=2).transpose(1, 2).reshape(-1, 2 * C * 4)
    assert torch.equal(rows.cpu().float(), want)
    # unpatchify on rows that differ between the two samples (patchify's are two copies of one latent)
    rows2 = randbf(g, *rows.shape)
    back = ops.unpatchify(rows2.to(DEV), B, Fr, 2 * C, H, W).cpu().float()
    want2 = F.fold(rows2.float().view(B * Fr, (H // 2) * (W // 2), 2 * C * 4).transpose(1, 2), (H, W), kernel_size=2, stride=2).view(B, Fr, 2 * C, H, W)
    assert torch.equal(back, want2)
    assert torch.equal(ops.unpatchify(rows, B, Fr, 2 * C, H, W).cpu().float(), x)


# ---------------------------------------------------------------------------------------------- cap 4 096 workgroups (unet_ops.hip)
IM2COL = [(64, 2, 72, 128, 1, False),     # Kpad = 576 = 9C: 18 432 rows x 72 vectors = 1 327 104 vectors = 1 sweep of 1 048 576 + 278 528
          (64, 2, 72, 128, 2, False),     # 4 608 rows x 72 = 331 776 vectors: the issue's shape at stride 2 stays inside one sweep (odd-tap arithmetic at size) ...
          (64, 8, 72, 128, 2, False),     # ... so the same at N = 8: 1 327 104 vectors = 1 sweep + 278 528
          (64, 4, 36, 64, 1, True),       # upsample (H, W halved, N doubled): 36 864 rows x 72 = 2 654 208 vectors = 2 sweeps + 557 056
          (8, 2, 160, 256, 1, False),     # Kpad = 128 against 9C = 72: 81 920 rows x 16 vectors = 1 310 720 vectors = 1 sweep + 262 144; 7 zero pad vectors per row
          (8, 2, 160, 256, 2, False),     # 20 480 rows x 16 = 327 680 vectors: inside one sweep, as above ...
          (8, 8, 160, 256, 2, False),     # ... and at N = 8: 1 310 720 vectors = 1 sweep + 262 144
          (8, 4, 80, 128, 1, True)]       # upsample (halved / doubled): 163 840 rows x 16 = 2 621 440 vectors = 2 sweeps + 524 288


@pytest.mark.parametrize("C,N,H,W,stride,up", IM2COL)
def test_im2col3x3_past_the_grid_cap(hip, C, N, H, W, stride, up):
    """im2col3x3_kernel, cap 4 096 workgroups = 1 048 576 vectors per sweep (per case: IM2COL).  Bit-exact against F.unfold on the (nearest-upsampled) input,
    reordered from unfold's (c, ky, kx) columns to the kernel's (ky, kx, c); the columns [9C, Kpad) must be zero."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(C + N + stride + up)
    x = randbf(g, N, H, W, C)
    got = ops.im2col3x3(x.to(DEV), stride=stride, upsample=up).cpu()
    xin = x.float().permute(0, 3, 1, 2)
    if up:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    cols = F.unfold(xin, kernel_size=3, padding=1, stride=stride)                     # [N, C * 9, L], column (c, ky, kx)
    L = cols.shape[2]
    want = cols.view(N, C, 9, L).permute(0, 3, 2, 1).reshape(N * L, 9 * C)
    kp = (9 * C + 63) // 64 * 64
    assert got.shape == (N * L, kp)
    assert torch.equal(got[:, :9 * C].float(), want)
    assert not got[:, 9 * C:].view(torch.int16).any()                                 # (bit pattern: the pad is +0, not -0)


def test_unfold_t3_past_the_grid_cap(hip):
    """unfold_t3_kernel, cap 4 096 workgroups: B = 2, T = 5, HW = 2 304, C = 320 -> 23 040 rows x 120 vectors = 2 764 800 vectors = two sweeps of 1 048 576 +
    667 648.  Sample 0's last frame and all of sample 1 lie behind the first sweep: their zero taps (kt = 0 of a first frame, kt = 2 of a last one) are
    checked explicitly besides the bit-exact gather."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(117)
    B, T, HW, C = 2, 5, 2304, 320
    x = randbf(g, B, T, HW, C)
    got = ops.unfold_t3(x.view(B * T, HW, C).to(DEV), B, T).cpu().view(B, T, HW, 3, C)
    pad = F.pad(x, (0, 0, 0, 0, 1, 1))                                                # zero frames in front of and behind each sample
    want = torch.stack([pad[:, kt:kt + T] for kt in range(3)], dim=3)
    assert torch.equal(got, want)
    assert not got[:, 0, :, 0].view(torch.int16).any() and not got[:, T - 1, :, 2].view(torch.int16).any()
    assert torch.equal(got[1, 0, :, 1], x[1, 0]) and torch.equal(got[0, T - 1, :, 0], x[0, T - 2])


def test_geglu_past_the_grid_cap(hip):
    """geglu_kernel, cap 4 096 workgroups: rows 9 216, inner 1 280 -> 1 474 560 vectors = one sweep of 1 048 576 + 425 984 (the gate is read at column offset
    `inner` of a row twice as wide as the output's)"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(118)
    y = randbf(g, 9216, 2 * 1280)
    a, gate = y.float().chunk(2, dim=-1)
    close(ops.geglu(y.to(DEV)), a * F.gelu(gate))


@pytest.mark.parametrize("with_noise", [True, False])
def test_ddim_v_step_past_the_grid_cap(hip, with_noise):
    """ddim_v_kernel, cap 4 096 workgroups, one fp32 element per thread: n = 2 * 4 * 16 * 72 * 128 = 1 179 648 = one sweep of 1 048 576 + 131 072.  Against an
    fp64 restatement of samplers/ddim.py's update (conditional half first) on the coefficients of a mid-schedule step (test_gpu_dc_sampler._coeffs, as the
    C ABI's floats hold them)."""
    from motionrag_amd import ops
    from test_gpu_dc_sampler import _coeffs
    g = torch.Generator().manual_seed(119)
    shape = (2, 4, 16, 72, 128)
    v, x, noise = randbf(g, 2, *shape), torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
    sa, sb, rescale, sqrt_aprev, dir_coef, sigma = (f32(c) for c in _coeffs())
    s = f32(7.5)
    got = ops.ddim_v_step_(v.to(DEV), x.to(DEV).clone(), noise.to(DEV) if with_noise else None, s, sa, sb, rescale, sqrt_aprev, dir_coef, sigma)
    assert got.dtype == torch.float32
    vc, vu, xx = v[0].double(), v[1].double(), x.double()
    vv, mv = vu + s * (vc - vu), vu.abs() + s * (vc.abs() + vu.abs())
    eps, x0 = sa * vv + sb * xx, (sa * xx - sb * vv) * rescale
    exact = sqrt_aprev * x0 + dir_coef * eps + (sigma * noise.double() if with_noise else 0.0)
    m = abs(sqrt_aprev * rescale) * ((sa * xx).abs() + sb * mv) + abs(dir_coef) * (sa * mv + (sb * xx).abs()) + ((sigma * noise.double()).abs() if with_noise else 0.0)
    bounded(f"ddim_v_step_ noise={with_noise}", got, exact, m, rel=0.0, sweep=SWEEP_4096)


# ---------------------------------------------------------------------------------------------- GroupNorm apply: cap max(4096 / N, 16) workgroups per sample
@pytest.mark.parametrize("N,HW,C,silu,use_emb", [(64, 600, 960, True, True), (256, 160, 960, False, False)])
def test_groupnorm_apply_past_the_grid_cap(hip, N, HW, C, silu, use_emb):
    """gn_apply_kernel walks runs of 1 024 vectors per workgroup and carries its channel-vector index by `ustep` (per unrolled vector), `rstep` (per grid stride
    of runs) and `cstep` (tail) with conditional subtracts; C / 8 = 120 (a skip-concat width) is no power of two.
    N = 64, HW = 600: 72 000 vectors per sample against a cap of 64 workgroups -> 70 whole runs: workgroups 0 .. 5 walk two (rstep = 64 * 1024 mod 120 = 16),
    then a 320-vector tail.  N = 256, HW = 160: the floor of 16 workgroups, 19 200 vectors -> 18 runs (two for workgroups 0 and 1) + a 768-vector tail.
    Reference: F.group_norm in fp32 on x + emb; the shipped three-launch form (statistics, fold, apply) is the one under test."""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(N + C)
    x = randbf(g, N, HW, C, scale=1.5, shift=0.3)
    w, b = randbf(g, C, scale=0.2, shift=1.0), randbf(g, C, scale=0.2)
    emb = randbf(g, N, C) if use_emb else None
    with ops.dispatched() as d:
        got = ops.groupnorm(x.to(DEV), w.to(DEV), b.to(DEV), 32, 1e-5, silu=silu, emb=emb.to(DEV) if use_emb else None)
    assert d.counts == {"GN_STATS": 1, "GN_FOLD": 1, "GN_APPLY": 1}, d.counts
    xin = x.float() + (emb.float()[:, None] if use_emb else 0)
    want = F.group_norm(xin.permute(0, 2, 1), 32, w.float(), b.float(), 1e-5).permute(0, 2, 1)
    close(got, F.silu(want) if silu else want)


# ---------------------------------------------------------------------------------------------- cap 8 192 workgroups
@pytest.mark.parametrize("B,H,text_len,thw", [(2, 12, 10, (5, 28, 30)), (2, 3, 10, (5, 40, 42))])
def test_qknorm_rope_past_the_grid_cap(hip, B, H, text_len, thw):
    """qknorm_rope_kernel, cap 8 192 workgroups x 4 waves = 32 768 units per sweep, a unit = (token, q or k, group of 8 heads) re-derived per stride.
    H = 12, S = 10 + 5 * 28 * 30 = 4 210: two head groups, the second half empty -> 2 * 4 210 * 2 * 2 = 33 680 units = one sweep + 912.
    H = 3, S = 10 + 5 * 40 * 42 = 8 410: one group with five idle heads -> 33 640 units = one sweep + 872.  The reference path of test_qknorm_rope."""
    from motionrag_amd import ops
    from oracle import cama_ref, cogvideox_ref
    g = torch.Generator().manual_seed(H)
    S = text_len + thw[0] * thw[1] * thw[2]
    qkv = randbf(g, B, S, 3, H, 64)
    qg, qb, kg, kb = (randbf(g, 64, scale=0.2, shift=1.0) for _ in range(4))
    cos, sin = cogvideox_ref.rope_3d(64, *thw)
    got = ops.qknorm_rope_(qkv.reshape(B, S, 3 * H * 64).to(DEV).clone(), H, qg.to(DEV), qb.to(DEV), kg.to(DEV), kb.to(DEV), cos.to(DEV), sin.to(DEV),
                           text_len, eps=1e-6, q_premul=0.37).view(B, S, 3, H, 64).cpu()
    for which, (gm, bt, mul) in enumerate(((qg, qb, 0.37), (kg, kb, 1.0))):
        x = cama_ref.layer_norm(qkv[:, :, which].float(), gm.float(), bt.float(), 1e-6).permute(0, 2, 1, 3).clone()        # [B, H, S, 64]
        x[:, :, text_len:] = cogvideox_ref.apply_rotary_emb(x[:, :, text_len:], cos, sin)
        close(got[:, :, which], (x * mul).permute(0, 2, 1, 3))
    assert torch.equal(got[:, :, 2], qkv[:, :, 2])                                    # V untouched, bit for bit


@pytest.mark.parametrize("P,with_pos", [(1, True), (1, False), (0, True)])
def test_assemble_tokens_past_the_grid_cap(hip, P, with_pos):
    """assemble_tokens_kernel, cap 8 192 workgroups = 2 097 152 vectors per sweep: N = 16, L = 1 369, D = 1 024 -> 16 * (1 369 + P) * 128 = 2 805 760 vectors
    with the class token (P = 1; one sweep + 708 608), 2 803 712 without (P = 0; one sweep + 706 560)"""
    from motionrag_amd.encoders import assemble_tokens
    g = torch.Generator().manual_seed(120 + P)
    N, L, D = 16, 1369, 1024
    x = randbf(g, N, L, D)
    prefix = randbf(g, P, D) if P else None
    pos = randbf(g, L + P, D) if with_pos else None
    got = assemble_tokens(x.to(DEV), prefix.to(DEV) if P else None, pos.to(DEV) if with_pos else None)
    a = torch.cat([prefix[None].expand(N, P, D), x], dim=1).double() if P else x.double()
    p = pos.double()[None] if with_pos else torch.zeros(1, L + P, D, dtype=torch.float64)
    bounded(f"assemble_tokens P={P} pos={with_pos}", got, a + p, a.abs() + p.abs(), sweep=8 * 8192 * 256)


# ---------------------------------------------------------------------------------------------- cap 16 384 workgroups
def test_blend_tile_past_the_grid_cap(hip):
    """blend_tile_kernel, cap 16 384 workgroups = 4 194 304 elements per sweep: T = 3, th = 96, tw = 120, C = 128 -> 4 423 680 elements = one sweep + 229 376
    (frame 2 from row 81 on: its horizontal band runs in the second sweep; the vertical band and the corner in the first).  Tile above and tile to the left given, extents (5, 12); against the oracle loops of
    test_blend_tile_matches_oracle_loops in fp64, the vertical blend rounded to bf16 where the horizontal one follows (the kernel's contract: the reference
    blends a bf16 tensor in place twice; module docstring for the rounding's bracket).  Outside the seam bands the tile keeps its bits."""
    from motionrag_amd import ops
    from oracle import cogvideox_vae_ref as R
    g = torch.Generator().manual_seed(121)
    T, th, tw, C, ev, eh = 3, 96, 120, 128, 5, 12
    tile, up, left = randbf(g, T, th, tw, C), randbf(g, T, 7, tw, C), randbf(g, T, th, 20, C)
    got = ops.blend_tile(tile.to(DEV).clone(), up.to(DEV), left.to(DEV), ev, eh).cpu()
    o5 = lambda t: t.double().permute(3, 0, 1, 2)[None].contiguous()                  # [T, h, w, C] -> the oracle's [1, C, T, h, w]
    back = lambda t: t[0].permute(1, 2, 3, 0)
    v = R._blend_v(o5(up), o5(tile), ev)
    mv = R._blend_v(o5(up).abs(), o5(tile).abs(), ev)
    ok_v, ratio_v = within(got, back(v), back(mv))                                    # rows above the horizontal band: one expression, one rounding
    # the horizontal blend of the rounded intermediate: within the bound of either end of its bracket (nearly always one value, else two neighbours), or --
    # where the vertical blend cancelled and the bracket holds more bf16 values than its ends -- between the ends (the blend is monotone in it: weights >= 0)
    lo, hi = bf(v - FP32_SLACK * mv).double(), bf(v + FP32_SLACK * mv).double()
    ends = []
    for cand in (lo, hi):
        h = back(R._blend_h(o5(left), cand.clone(), eh))
        mh = back(R._blend_h(o5(left).abs(), cand.abs(), eh))
        ends.append((h, HALF_ULP * h.abs() + FP32_SLACK * mh))
    ulp = torch.ldexp(torch.ones_like(hi), torch.frexp(torch.maximum(lo.abs(), hi.abs()))[1] - 8)       # bf16 spacing at the larger end
    g64 = got.double()
    inside = back(hi - lo > ulp) & (g64 >= ends[0][0] - ends[0][1]) & (g64 <= ends[1][0] + ends[1][1])
    ok_h = ((g64 - ends[0][0]).abs() <= ends[0][1]) | ((g64 - ends[1][0]).abs() <= ends[1][1]) | inside
    in_h = torch.zeros(T, th, tw, C, dtype=torch.bool)
    in_h[:, :, :eh] = True
    print(f"blend_tile: worst element outside the horizontal band at {ratio_v[~in_h].max().item():.3f} x the bound")
    bounded("blend_tile", got, back(v), back(mv), sweep=16384 * 256, ok=torch.where(in_h, ok_h, ok_v))
    assert torch.equal(got[:, ev:, eh:], tile[:, ev:, eh:])
    # (what the bands must NOT be: the input)
    assert not torch.equal(got[:, :ev], tile[:, :ev]) and not torch.equal(got[:, :, :eh], tile[:, :, :eh])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_denormalize_past_the_grid_cap(hip, dtype):
    """denormalize_u8_kernel, cap 16 384 workgroups, one element per thread: 3 x 17 x 288 x 512 = 7 520 256 elements = one sweep of 4 194 304 + 3 325 952.
    Bit-exact against the reference's torch ops on the host (test_gpu_harness.ref_denormalize)."""
    from motionrag_amd.eval_harness import denormalize
    from test_gpu_harness import ref_denormalize
    g = torch.Generator().manual_seed(122)
    x = (torch.randn(3, 17, 288, 512, generator=g) * 0.8).to(dtype)
    got = denormalize(x.to(DEV)).cpu()
    want = ref_denormalize(x)
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), int((got != want).sum())


# ---------------------------------------------------------------------------------------------- refusals
def test_misaligned_views_are_refused_not_processed(hip):
    """the vector kernels read 16 bytes per lane: a view that starts 2 bytes into an allocation (`x.view(-1)[1:]`) must be refused by the wrapper or by the
    C ABI (MRAG_EINVAL) for silu, add, axpby and add_bcast, and the output buffer must keep its contents"""
    from motionrag_amd import ops
    g = torch.Generator().manual_seed(123)
    n, D = 4096, 64
    base, other, tab = randbf(g, n + 1).to(DEV), randbf(g, n + 1).to(DEV), randbf(g, 3, D).to(DEV)
    base0 = base.clone()
    x, y = base.view(-1)[1:], other.view(-1)[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 == 2
    aligned = other[:n]
    out = torch.full((n,), 7.0, dtype=torch.bfloat16, device=DEV)
    refused(lambda: ops.silu(x))
    for a, b in ((x, y), (x, aligned), (aligned, y)):
        refused(lambda: ops.add(a, b, out=out))
        refused(lambda: ops.axpby(a, b, 0.5, 0.5, out=out))
    refused(lambda: ops.add(aligned, aligned.clone(), out=x))
    refused(lambda: ops.add_bcast(x.view(n // D, D), tab, 4, out=out.view(n // D, D)))
    refused(lambda: ops.add_bcast(aligned.view(n // D, D), tab, 4, out=x.view(n // D, D)))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(base, base0)
    close(ops.silu(aligned), F.silu(aligned.float().cpu()))                           # (the aligned twin is taken)


def test_weighted_sum_and_cfg_euler_refuse_bad_shapes(hip):
    from motionrag_amd import ops
    with pytest.raises(ValueError):
        ops.weighted_sum(torch.zeros(2, 3, 5, 7, dtype=torch.bfloat16, device=DEV), None)          # 35 trailing elements: no multiple of 8
    with pytest.raises(ValueError):
        ops.weighted_sum(torch.zeros(2, 3, 4, dtype=torch.bfloat16, device=DEV), torch.ones(2, 3, device=DEV))
    lat = torch.zeros(1, 4, 2, 4, 8, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros(2, 1, 4, 2, 4, 8, dtype=torch.bfloat16, device=DEV)
    for bad in (3, 5, 8):
        with pytest.raises(ValueError):
            ops.cfg_euler_step_(v, lat, torch.ones(bad, device=DEV), 1.0, 0.5)                      # one guidance scale per frame (4) expected
    ops.cfg_euler_step_(v, lat, torch.ones(4, device=DEV), 1.0, 0.5)
    torch.cuda.synchronize()
