"""ORACLE TOOLING (runs where the reference tree is; never on the GPU box): the fixtures of the DynamiCrafter sampler options that
oracle/gen_golden.py does not pin -- 'uniform_trailing' timestep spacing, guidance rescale, the loop / interp conditioning -- made, like
G11 / G12 / G14 there, by driving the reference's OWN classes on the CPU and storing what they return.

    python -m tools.gen_dc_sampler_golden        # writes tests/golden/dc_sampler_trailing.npz and tests/golden/dc_pipeline_native.npz

Nothing else under tests/golden/ is touched: the helpers borrowed from oracle.gen_golden write their own fixtures into a scratch directory.

  dc_sampler_trailing.npz   make_ddim_timesteps('uniform_trailing', S, 1000) for S = 5, 25, 30, 50; make_ddim_sampling_parameters at S = 30,
                            eta 1; five p_sample_ddim steps at S = 5 (trailing, eta 1, CFG 2.0, guidance_rescale 0.7) on x [2, 4, 4, 8, 8] with
                            recorded noise.  The duck model is 0.5 x + field cos(t / 100) with a FULL-SHAPE random field per branch: a per-sample
                            constant (dc_schedule.npz) shifts cond and guided prediction alike, std(g) == std(v_c), and rescale does nothing.
  dc_pipeline_native.npz    the G14 set-up (reduced UNet with the G10 weights, stand-ins of oracle/stubs.py, 64 x 64, 4 frames, 5 steps, recorded
                            x_T and noises): (A) timestep_spacing='uniform_trailing', guidance_rescale=0.7; (B) interp=True on a clip whose last
                            frame differs from its first; each beside the same call with the option off (its control).
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PIPELINE_TOL = 5e-2            # the relative L2 bound of the pipeline tests; a recording must be three times that from its control


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a - b).norm() / b.norm())


def duck_tables(ac, betas):
    """the buffers DDIMSampler and p_sample_ddim read from the model (ddpm3d.py:134-198, 535-541)"""
    return dict(betas=torch.tensor(betas, dtype=torch.float32), alphas_cumprod=torch.tensor(ac, dtype=torch.float32),
                alphas_cumprod_prev=torch.tensor(np.append(1.0, ac[:-1]), dtype=torch.float32),
                sqrt_alphas_cumprod=torch.tensor(np.sqrt(ac), dtype=torch.float32),
                sqrt_one_minus_alphas_cumprod=torch.tensor(np.sqrt(1.0 - ac), dtype=torch.float32),
                scale_arr=torch.tensor(np.concatenate((np.linspace(1.0, 0.3, 400), np.full(1000, 0.3))), dtype=torch.float32))


def v_to_x0(self, x, t, v):                     # ddpm3d.py:251-256
    return self.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1, 1) * x - self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1, 1) * v


def v_to_eps(self, x, t, v):                    # ddpm3d.py:258-263
    return self.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1, 1) * v + self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1, 1) * x


def gen_sampler(ud, ddim_mod, ac, betas):
    ts = {S: ud.make_ddim_timesteps("uniform_trailing", S, 1000, verbose=False) for S in (5, 25, 30, 50)}
    sig, al, alp = ud.make_ddim_sampling_parameters(torch.tensor(ac, dtype=torch.float32), ts[30], 1.0, verbose=False)

    class Duck:
        num_timesteps, parameterization, use_dynamic_rescale, device = 1000, "v", True, torch.device("cpu")
        predict_start_from_z_and_v, predict_eps_from_z_and_v = v_to_x0, v_to_eps

        def __init__(self):
            self.alphas_cumprod_np = ac
            for k, v in duck_tables(ac, betas).items():
                setattr(self, k, v)

        def apply_model(self, x, t, c, **kw):
            return 0.5 * x + c["field"] * torch.cos(t.float() / 100.0).view(-1, 1, 1, 1, 1)

    smp = ddim_mod.DDIMSampler(Duck())
    smp.make_schedule(5, ddim_discretize="uniform_trailing", ddim_eta=1.0, verbose=False)
    gi = torch.Generator().manual_seed(510)
    shape = (2, 4, 4, 8, 8)
    xT = torch.randn(shape, generator=gi)
    c, uc = {"field": torch.randn(shape, generator=gi)}, {"field": torch.randn(shape, generator=gi)}
    xs, xs_plain, noises, x = [], [], [], xT
    steps = np.flip(smp.ddim_timesteps)
    for i in range(5):
        index = len(steps) - i - 1
        tsx = torch.full((2,), int(steps[i]), dtype=torch.long)
        torch.manual_seed(600 + i)
        noises.append(torch.randn(shape).numpy())
        torch.manual_seed(600 + i)
        x_next, _ = smp.p_sample_ddim(x, c, tsx, index=index, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, guidance_rescale=0.7)
        torch.manual_seed(600 + i)
        plain, _ = smp.p_sample_ddim(x, c, tsx, index=index, unconditional_guidance_scale=2.0, unconditional_conditioning=uc, guidance_rescale=0.0)
        assert torch.isfinite(x_next).all()
        xs.append(x_next.numpy()); xs_plain.append(plain.numpy())
        x = x_next
    gap = [float(np.abs(a - b).max()) for a, b in zip(xs, xs_plain)]
    print("trailing steps", steps.tolist(), "max |rescaled - plain| per step", ["%.3g" % g for g in gap])
    np.savez(os.path.join(OUT, "dc_sampler_trailing.npz"), t5=ts[5], t25=ts[25], t30=ts[30], t50=ts[50], sigmas=sig.numpy(), alphas=al.numpy(),
             alphas_prev=alp.numpy(), xT=xT.numpy(), c_field=c["field"].numpy(), uc_field=uc["field"].numpy(), noises=np.stack(noises), xs=np.stack(xs),
             guidance=np.float32(2.0), guidance_rescale=np.float32(0.7))


def gen_pipeline(inf, ddim_mod, res_mod, unet, ac, betas):
    from oracle import stubs

    class Wrapper(nn.Module):                       # DiffusionWrapper, conditioning_key 'hybrid' (ddpm3d.py:1378-1382)
        conditioning_key = "hybrid"

        def __init__(self, dm):
            super().__init__()
            self.diffusion_model = dm

        def forward(self, x, t, c_concat=None, c_crossattn=None, **kwargs):
            return self.diffusion_model(torch.cat([x] + c_concat, dim=1), t, context=c_crossattn, **kwargs)

    class DuckLVD(nn.Module):                       # what image_guided_synthesis and DDIMSampler read from LatentVisualDiffusion (as G14)
        num_timesteps, parameterization, use_dynamic_rescale, uncond_type = 1000, "v", True, "empty_seq"
        action_embedder = None
        device = torch.device("cpu")
        predict_start_from_z_and_v, predict_eps_from_z_and_v = v_to_x0, v_to_eps

        def __init__(self):
            super().__init__()
            self.model = Wrapper(unet)
            self.embedder = stubs.ImageEmbedderStub(tokens=9, dim=48)
            self.image_proj_model = res_mod.Resampler(dim=64, depth=2, dim_head=64, heads=2, num_queries=3, embedding_dim=48, output_dim=64, video_length=4).eval()
            gg.seeded_state(self.image_proj_model, 404, std=0.08)
            self.condition_transformer = stubs.ConditionTransformerStub(dim=64)
            self.first_stage = stubs.FirstStageStub()
            self.text = stubs.TextStub(tokens=7, dim=64)
            self.alphas_cumprod_np = ac
            for k, v in duck_tables(ac, betas).items():
                self.register_buffer(k, v)

        def get_learned_conditioning(self, prompts):
            return self.text(prompts)

        def encode_first_stage(self, x):
            return self.first_stage.encode_first_stage(x)

        def decode_first_stage(self, z):
            return self.first_stage.decode_first_stage(z)

        def apply_model(self, x_noisy, t, cond, **kwargs):       # ddpm3d.py:745-760 (dict branch)
            return self.model(x_noisy, t, **cond, **kwargs)

    model = DuckLVD().eval()
    gi = torch.Generator().manual_seed(505)
    b, T, H, W = 1, 4, 64, 64
    image = torch.rand(b, 3, H, W, generator=gi) * 2 - 1
    image_last = torch.rand(b, 3, H, W, generator=gi) * 2 - 1
    ref_videos = torch.rand(b, 3, T, 3, 16, 16, generator=gi) * 2 - 1
    prompts = ["a corgi running on the beach"]
    still = image[:, :, None].expand(-1, -1, T, -1, -1)                                  # DynamiCrafterPipelineRef.__call__ :95
    w = torch.linspace(0, 1, T).view(1, 1, T, 1, 1)
    clip = image[:, :, None] * (1 - w) + image_last[:, :, None] * w                     # first frame `image`, last frame `image_last`
    real_randn = torch.randn

    def run(videos, guidance, **opts):
        drawn = []

        def recording_randn(*a, **k):
            k.pop("device", None)
            v = real_randn(*a, **k)
            drawn.append(v.clone())
            return v

        torch.manual_seed(506)
        torch.randn = recording_randn
        try:
            with torch.no_grad():
                kw = dict(loop=False, interp=False, timestep_spacing="uniform", guidance_rescale=0.0)
                kw.update(opts)
                out = inf.image_guided_synthesis(model=model, prompts=prompts, videos=videos, noise_shape=[b, 4, T, H // 8, W // 8], n_samples=1, ddim_steps=5,
                                                 ddim_eta=1.0, unconditional_guidance_scale=guidance, cfg_img=None, fs=15, text_input=True,
                                                 multiple_cond_cfg=False, ref_videos=ref_videos, ref_fusion_type=None, metadata=None, **kw)
        finally:
            torch.randn = real_randn
        shape5 = [d for d in drawn if tuple(d.shape) == (b, 4, T, H // 8, W // 8)]
        assert len(shape5) == 6, [tuple(d.shape) for d in drawn]                         # x_T + one noise per DDIM step
        return out[:, 0].permute(0, 2, 1, 3, 4), torch.stack(shape5)                     # 'b 1 c t h w -> b t c h w'  (pipeline.py:115)

    for guidance in (2.0, 3.0, 4.0, 5.0, 7.5):
        a, draws = run(still, guidance, timestep_spacing="uniform_trailing", guidance_rescale=0.7)
        a_ctl, d1 = run(still, guidance)
        bb, d2 = run(clip, guidance, interp=True)
        b_ctl, d3 = run(clip, guidance)
        assert all(torch.equal(draws, d) for d in (d1, d2, d3))
        gaps = rel_l2(a, a_ctl), rel_l2(bb, b_ctl)
        print(f"guidance {guidance}: relative L2 to the control  (A) {gaps[0]:.3f}  (B) {gaps[1]:.3f}")
        if min(gaps) >= 3 * PIPELINE_TOL:
            break
    assert min(gaps) >= 3 * PIPELINE_TOL, gaps
    assert all(torch.isfinite(t).all() for t in (a, a_ctl, bb, b_ctl))
    np.savez_compressed(os.path.join(OUT, "dc_pipeline_native.npz"), image=image.numpy(), image_last=image_last.numpy(), ref_videos=ref_videos.numpy(),
                        prompt=np.array(prompts[0]), guidance=np.float32(guidance), x_T=draws[0].numpy(), noises=draws[1:].numpy(),
                        frames_trailing_rescaled=a.numpy(), frames_trailing_rescaled_control=a_ctl.numpy(), frames_interp=bb.numpy(),
                        frames_interp_control=b_ctl.numpy(), proj_meta=np.array(json.dumps(dict(seed=404, **gg.SEEDED_META[404]))))


def main():
    gg.install_stubs()
    torch.manual_seed(0)
    dc = f"{gg.REF}/src/projects/dynamicrafter/DynamiCrafter"
    pkg = types.ModuleType("dcroot"); pkg.__path__ = [dc]; sys.modules["dcroot"] = pkg
    attn_mod = importlib.import_module("dcroot.lvdm.modules.attention")
    res_mod = gg._load_file("ref_resampler", f"{gg.REF}/src/projects/condition/encoders/resampler.py")
    with tempfile.TemporaryDirectory() as scratch:            # gen_dynamicrafter rewrites G8-G12 wherever gg.OUT points: not into tests/golden/
        gg.OUT = scratch
        unet = gg.gen_dynamicrafter(attn_mod)                 # the reference UNetModel with the G10 weights (seed 208)
    ac, betas = gg.gen_dynamicrafter.tables
    ud = importlib.import_module("dcroot.lvdm.models.utils_diffusion")
    ddim_mod = importlib.import_module("dcroot.lvdm.models.samplers.ddim")
    inf = importlib.import_module("dcroot.scripts.evaluation.inference")
    ddim_mod.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)      # the reference forces .to("cuda")
    gen_sampler(ud, ddim_mod, ac, betas)
    gen_pipeline(inf, ddim_mod, res_mod, unet, ac, betas)
    for f in ("dc_sampler_trailing.npz", "dc_pipeline_native.npz"):
        print(f"  {f}: {os.path.getsize(os.path.join(OUT, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
