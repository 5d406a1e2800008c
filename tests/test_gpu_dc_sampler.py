"""GPU tests of the DynamiCrafter sampler options: guidance rescale (mrag_ddim_v_step_rescaled_f32: per-sample standard deviations of the conditional and the
guided prediction, then the DDIM update) and 'uniform_trailing' timestep spacing against the REFERENCE sampler's recorded steps, the kernel against an fp64
restatement, determinism / graph capture, and the pipeline glue (trailing + rescale, interp conditioning) against the reference's own image_guided_synthesis.
Fixtures: tests/golden/dc_sampler_trailing.npz, dc_pipeline_native.npz (tools/gen_dc_sampler_golden.py)."""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

from test_gpu_kernels import close
from test_gpu_models import close as close_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bf(x):
    return x.to(torch.bfloat16)


def outside(got, want, scale=1.0, rtol=2e-2, atol_frac=2e-2):
    """elements of `got` that `close(got, want, scale)` would reject"""
    err = (got.float().cpu() - want.float().cpu()).abs()
    return int((err > rtol * want.float().cpu().abs() + atol_frac * scale).sum())


# ------------------------------------------------------------------------------------------------------------------------ 1. the reference's steps
def test_trailing_rescaled_ddim_steps_against_reference_golden(hip, golden_dir):
    """five eta = 1 DDIM steps on the trailing schedule (t = 999, 799, .., 199; CFG 2.0, guidance_rescale 0.7, dynamic rescale, recorded CPU noise) vs
    DDIMSampler.p_sample_ddim, under the bound of test_dc_ddim_steps_against_reference_golden (2 % + 0.02: v is fed in bf16; an fp64 restatement on the same
    tables and bf16 inputs sits at <= 1.5e-2).  The same steps WITHOUT the rescale must miss that bound, every one of them: the fixture's duck model has a
    full-shape field per branch, so std(g) != std(v_c)."""
    from motionrag_amd import ops
    from motionrag_amd.dynamicrafter import DDIMSampler
    g = np.load(os.path.join(golden_dir, "dc_sampler_trailing.npz"))
    smp = DDIMSampler()
    np.testing.assert_array_equal(smp.make_schedule(5, 1.0, "uniform_trailing"), g["t5"])
    x = torch.from_numpy(g["xT"]).to(DEV)
    c, uc = torch.from_numpy(g["c_field"]), torch.from_numpy(g["uc_field"])
    n = len(smp.ddim_timesteps)
    for i in range(5):
        t, sa, sb, rescale, sqrt_aprev, dir_coef, sigma = smp.step_coeffs(n - 1 - i)
        f = math.cos(t / 100.0)
        xc = x.cpu()
        v = bf(torch.cat([0.5 * xc + c * f, 0.5 * xc + uc * f], dim=0)).to(DEV).contiguous()      # the duck-typed model of the fixture
        noise, want = torch.from_numpy(g["noises"][i]).to(DEV), torch.from_numpy(g["xs"][i])
        plain = ops.ddim_v_step_(v, x.clone(), noise, 2.0, sa, sb, rescale, sqrt_aprev, dir_coef, sigma)
        ops.ddim_v_step_rescaled_(v, x, noise, 2.0, 0.7, sa, sb, rescale, sqrt_aprev, dir_coef, sigma)
        print(f"step {i} t {t}: max err rescaled {(x.cpu() - want).abs().max().item():.4g}, plain {(plain.cpu() - want).abs().max().item():.4g} "
              f"({outside(plain, want)} elements outside)")
        close(x, want, scale=1.0)
        assert outside(plain, want) > 0, f"step {i}: the un-rescaled update passes the bound -- the fixture shows nothing"
        x = want.to(DEV)                                                                            # re-anchor: v is fed in bf16


# ------------------------------------------------------------------------------------------------------------------------ 2. kernel vs fp64
def _coeffs():
    from motionrag_amd.dynamicrafter import DDIMSampler
    smp = DDIMSampler()
    smp.make_schedule(30, 1.0, "uniform_trailing")
    return smp.step_coeffs(17)[1:]                                   # a mid-schedule step: every coefficient of the update is O(0.1 .. 1)


@pytest.mark.parametrize("n", [2, 255, 257, 1024, 4 * 16 * 72 * 128])
@pytest.mark.parametrize("batch", [1, 2, 3])
def test_rescaled_step_against_fp64_restatement(hip, batch, n):
    """sample s is scaled by s + 1 and shifted by +4: statistics taken from the wrong sample, or by a cancelling sum of squares, both show.  589 824 is the
    production element count (a reduction's error grows with its length).  |got - want| <= 1e-5 (1 + |want|): a dozen fp32 roundings and a tree sum, 15 x
    over what an fp32 torch restatement leaves (<= 6.6e-7 on O(1) values); var = E[x^2] - mean^2 in one fp32 pass (17 - 16 here, over 589 824 terms) does
    not fit in it.  Measured: the kernel's worst element is at 0.13 x the bound (batch 3, n 589 824), 0.07 x and below at the short sizes."""
    from motionrag_amd import ops
    gen = torch.Generator().manual_seed(1000 * batch + n % 997)
    scale = torch.arange(1, batch + 1, dtype=torch.float32).repeat(2).view(2 * batch, 1)
    v = bf(torch.randn(2 * batch, n, generator=gen) * scale + 4.0)
    x0, noise = torch.randn(batch, n, generator=gen), torch.randn(batch, n, generator=gen)
    sa, sb, rescale, sqrt_aprev, dir_coef, sigma = _coeffs()
    vd, xd, nd = v.to(DEV), x0.to(DEV), noise.to(DEV)
    vc, vu = v[:batch].double(), v[batch:].double()
    worst = 0.0
    for guidance in (2.0, 7.5):
        gd = vu + guidance * (vc - vu)
        r = vc.std(dim=1, keepdim=True) / gd.std(dim=1, keepdim=True)
        for phi in (0.7, 1.0):
            phi32 = float(np.float32(phi))                           # what the C ABI's float argument holds
            vv = phi32 * (gd * r) + (1.0 - phi32) * gd
            eps, px0 = sa * vv + sb * x0.double(), (sa * x0.double() - sb * vv) * rescale
            for with_noise in (True, False):
                want = sqrt_aprev * px0 + dir_coef * eps + (sigma * noise.double() if with_noise else 0.0)
                got = ops.ddim_v_step_rescaled_(vd, xd.clone(), nd if with_noise else None, guidance, phi, sa, sb, rescale, sqrt_aprev, dir_coef, sigma)
                assert torch.isfinite(got).all()
                ratio = ((got.cpu().double() - want).abs() / (1e-5 * (1.0 + want.abs()))).max().item()
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"guidance {guidance} phi {phi} noise {with_noise}: {ratio:.3g} x the bound"
    print(f"batch {batch} n {n}: worst error {worst:.3g} x the bound")


def test_rescaled_step_layout_errors(hip):
    from motionrag_amd import ops
    x = torch.zeros(2, 4, 8, device=DEV)
    v = torch.zeros(4, 4, 8, device=DEV, dtype=torch.bfloat16)
    args = (2.0, 0.7, 0.5, 0.5, 1.0, 0.9, 0.1, 0.2)
    ops.ddim_v_step_rescaled_(v, x, None, *args)
    with pytest.raises(ValueError):
        ops.ddim_v_step_rescaled_(v[:3], x, None, *args)                                    # not [2b, ...]
    with pytest.raises(ValueError):
        ops.ddim_v_step_rescaled_(v.transpose(1, 2), x.transpose(1, 2), None, *args)        # not contiguous
    with pytest.raises(ValueError):
        ops.ddim_v_step_rescaled_(v, x, torch.zeros(2, 4, 4, device=DEV), *args)            # noise of another shape
    with pytest.raises(TypeError):
        ops.ddim_v_step_rescaled_(v.float(), x, None, *args)
    from motionrag_amd._lib import HipError
    with pytest.raises(HipError):
        ops.ddim_v_step_rescaled_(v, x, None, 2.0, 0.0, *args[2:])                          # guidance_rescale 0 belongs to ddim_v_step_


# ------------------------------------------------------------------------------------------------------------------------ 3. determinism, capture
def test_rescaled_step_is_deterministic_and_captures(hip):
    """two launches, no host synchronisation, nothing read back: two runs are bit-equal, and a captured graph replays to the eager result"""
    from motionrag_amd import ops
    gen = torch.Generator().manual_seed(5)
    b, n = 2, 70001                                                   # 69 partials per sample, an odd tail
    v = bf(torch.randn(2 * b, n, generator=gen) * 2 + 1).to(DEV)
    x0, noise = torch.randn(b, n, generator=gen).to(DEV), torch.randn(b, n, generator=gen).to(DEV)
    c = _coeffs()
    run = lambda x: ops.ddim_v_step_rescaled_(v, x, noise, 7.5, 0.7, *c)
    eager = run(x0.clone())                                           # warm: the workspace is grown
    assert torch.equal(run(x0.clone()), eager)
    assert not torch.equal(eager, ops.ddim_v_step_(v, x0.clone(), noise, 7.5, *c))
    xg = x0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.HIPGraph() if hasattr(torch.cuda, "HIPGraph") else torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(xg)
    xg.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(xg, eager)


def test_sample_without_rescale_is_todays_loop(hip):
    """`sample(..., guidance_rescale=0.0)` on the default spacing launches what it launched before the options existed: bit-equal to the loop over
    step_coeffs + ops.ddim_v_step_; with the options on, the same loop over ops.ddim_v_step_rescaled_ on the trailing schedule"""
    from motionrag_amd import ops
    from motionrag_amd.dynamicrafter import DDIMSampler
    gen = torch.Generator().manual_seed(8)
    shape = (2, 4, 4, 8, 8)
    xT = torch.randn(shape, generator=gen).to(DEV)
    field = bf(torch.randn(4, *shape[1:], generator=gen)).to(DEV)
    noises = [torch.randn(shape, generator=gen).to(DEV) for _ in range(5)]
    model = lambda x, t, cond, uncond: (bf(0.5 * x).repeat(2, 1, 1, 1, 1) + field * math.cos(t / 100.0)).contiguous()
    for spacing, phi in (("uniform", 0.0), ("uniform_trailing", 0.7)):
        smp = DDIMSampler()
        kw = {} if phi == 0.0 else dict(timestep_spacing=spacing, guidance_rescale=phi)
        got = smp.sample(model, xT.clone(), None, None, S=5, eta=1.0, unconditional_guidance_scale=2.0, noises=noises, **kw)
        ref = DDIMSampler()
        ref.make_schedule(5, 1.0, spacing)
        x = xT.clone()
        for i in range(5):
            t, *c = ref.step_coeffs(4 - i)
            v = model(x, t, None, None)
            if phi == 0.0:
                ops.ddim_v_step_(v, x, noises[i], 2.0, *c)
            else:
                ops.ddim_v_step_rescaled_(v, x, noises[i], 2.0, phi, *c)
        assert torch.isfinite(got).all() and torch.equal(got, x), spacing
    same = DDIMSampler().sample(model, xT.clone(), None, None, S=5, eta=1.0, unconditional_guidance_scale=2.0, noises=noises, timestep_spacing="uniform",
                                guidance_rescale=0.0)
    first = DDIMSampler().sample(model, xT.clone(), None, None, S=5, eta=1.0, unconditional_guidance_scale=2.0, noises=noises)
    assert torch.equal(same, first)


# ------------------------------------------------------------------------------------------------------------------------ 4. pipeline
@pytest.fixture(scope="module")
def native(hip, golden_dir):
    """the G14 set-up of test_dc_pipeline_glue_against_reference_golden: reduced UNet (dc_unet.npz weights), the stand-ins of oracle/stubs.py"""
    from motionrag_amd import cama, dynamicrafter as dc
    from oracle import stubs
    from oracle.seeded import seeded_sd
    from test_oracle_golden import dc_unet_fixture
    g = np.load(os.path.join(golden_dir, "dc_pipeline_native.npz"))
    _, sd, _, _, _ = dc_unet_fixture(golden_dir)
    unet = dc.UNetModel(in_channels=8, out_channels=4, model_channels=64, attention_resolutions=(1, 2), num_res_blocks=1, channel_mult=(1, 2),
                        num_head_channels=64, transformer_depth=1, context_dim=64, use_linear=True, temporal_conv=True, temporal_attention=True,
                        temporal_self_att_only=True, use_relative_position=False, temporal_length=4, addition_attention=True,
                        image_cross_attention=True, action_cross_attention=True, default_fs=10, fs_condition=True)
    unet.load_state_dict(sd, strict=True)
    unet = unet.to(DEV, torch.bfloat16)
    pm = json.loads(str(g["proj_meta"]))
    proj = cama.Resampler(dim=64, depth=2, dim_head=64, heads=2, num_queries=3, embedding_dim=48, output_dim=64, video_length=4)
    proj.load_state_dict(seeded_sd(pm["keys"], pm["shapes"], pm["seed"], pm["std"]), strict=True)
    fs_stub = stubs.FirstStageStub().to(DEV)
    model = types.SimpleNamespace(
        model=types.SimpleNamespace(conditioning_key="hybrid", diffusion_model=unet), uncond_type="empty_seq", action_embedder=None,
        embedder=stubs.ImageEmbedderStub(tokens=9, dim=48).to(DEV), image_proj_model=proj.to(DEV, torch.bfloat16),
        condition_transformer=stubs.ConditionTransformerStub(dim=64).to(DEV), get_learned_conditioning=stubs.TextStub(tokens=7, dim=64, device=DEV),
        encode_first_stage=fs_stub.encode_first_stage, decode_first_stage=fs_stub.decode_first_stage)
    return g, model


def _rel_l2(got, want):
    return ((got.float().cpu() - want).norm() / want.norm()).item()


def test_pipeline_trailing_rescaled_against_reference_golden(native):
    """recording (A): DynamiCrafterPipelineRef(timestep_spacing='uniform_trailing', guidance_rescale=0.7) vs the reference's image_guided_synthesis, under the
    bound of test_dc_pipeline_glue_against_reference_golden (five chained bf16 steps against the fp32 reference); the recorded control (options off) is at
    least three times that bound away, and the output must stay farther than the bound from it"""
    from motionrag_amd.dynamicrafter_pipeline import DynamiCrafterPipelineRef
    g, model = native
    pipe = DynamiCrafterPipelineRef(model)
    call = dict(image=torch.from_numpy(g["image"]).to(DEV), positive_prompt=[str(g["prompt"])], negative_prompt=None, height=64, width=64, num_frames=4,
                num_inference_steps=5, eta=1.0, unconditional_guidance_scale=float(g["guidance"]), frame_stride=15,
                ref_videos=torch.from_numpy(g["ref_videos"]).to(DEV), x_T=torch.from_numpy(g["x_T"]), noises=[torch.from_numpy(n) for n in g["noises"]])
    frames = pipe(timestep_spacing="uniform_trailing", guidance_rescale=0.7, **call)
    want, control = torch.from_numpy(g["frames_trailing_rescaled"]), torch.from_numpy(g["frames_trailing_rescaled_control"])
    assert frames.shape == want.shape == (1, 4, 3, 64, 64)
    print(f"(A) relative L2 to the recording {_rel_l2(frames, want):.4f}, to the control {_rel_l2(frames, control):.4f}")
    close_model(frames, want, rel_l2=5e-2, atol_frac=0.35)
    assert _rel_l2(frames, control) > 5e-2
    with pytest.raises(NotImplementedError):
        pipe(**dict(call, multiple_cond_cfg=True))
    with pytest.raises(NotImplementedError):
        pipe(**dict(call, timestep_spacing="quad"))


def test_pipeline_interp_against_reference_golden(native):
    """recording (B): image_guided_synthesis(interp=True) on a clip whose last frame differs from its first (c_concat = first and last latent frame, zeros
    between: inference.py:228-231), uniform spacing, no rescale"""
    from motionrag_amd.dynamicrafter_pipeline import image_guided_synthesis
    g, model = native
    image, last = torch.from_numpy(g["image"]), torch.from_numpy(g["image_last"])
    w = torch.linspace(0, 1, 4).view(1, 1, 4, 1, 1)
    clip = image[:, :, None] * (1 - w) + last[:, :, None] * w                                   # as the fixture's generator builds it
    call = dict(model=model, prompts=[str(g["prompt"])], videos=clip.to(DEV), noise_shape=[1, 4, 4, 8, 8], n_samples=1, ddim_steps=5, ddim_eta=1.0,
                unconditional_guidance_scale=float(g["guidance"]), fs=15, text_input=True, ref_videos=torch.from_numpy(g["ref_videos"]).to(DEV),
                x_T=torch.from_numpy(g["x_T"]), noises=[torch.from_numpy(n) for n in g["noises"]])
    out = image_guided_synthesis(interp=True, **call)
    assert out.shape == (1, 1, 3, 4, 64, 64)
    frames = out[:, 0].permute(0, 2, 1, 3, 4)
    want, control = torch.from_numpy(g["frames_interp"]), torch.from_numpy(g["frames_interp_control"])
    print(f"(B) relative L2 to the recording {_rel_l2(frames, want):.4f}, to the control {_rel_l2(frames, control):.4f}")
    close_model(frames, want, rel_l2=5e-2, atol_frac=0.35)
    assert _rel_l2(frames, control) > 5e-2
    assert torch.equal(image_guided_synthesis(loop=True, **call), out)                          # loop takes the same conditioning
    with pytest.raises(NotImplementedError):
        image_guided_synthesis(interp=True, multiple_cond_cfg=True, **call)
