"""CPU suite of the DynamiCrafter sampler options (no compute calls): 'uniform_trailing' timestep tables against the reference's recorded
ones (tests/golden/dc_sampler_trailing.npz, made by tools/gen_dc_sampler_golden.py from the reference's make_ddim_timesteps /
make_ddim_sampling_parameters), the unchanged default, the spacings that stay refused, and the C ABI of the guidance-rescale step."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_trailing_tables_match_reference_golden():
    from motionrag_amd.dynamicrafter import DDIMSampler
    g = np.load(os.path.join(GOLDEN, "dc_sampler_trailing.npz"))
    s = DDIMSampler()
    for S in (5, 25, 50):
        np.testing.assert_array_equal(s.make_schedule(S, 0.0, "uniform_trailing"), g[f"t{S}"])
    ts = s.make_schedule(30, 1.0, "uniform_trailing")
    np.testing.assert_array_equal(ts, g["t30"])
    assert ts[-1] == 999 and len(ts) == 30                          # the zero-SNR step is sampled
    np.testing.assert_allclose(s.ddim_sigmas, g["sigmas"], rtol=1e-6); np.testing.assert_allclose(s.ddim_alphas, g["alphas"], rtol=1e-6)
    np.testing.assert_allclose(s.ddim_alphas_prev, g["alphas_prev"], rtol=1e-6)
    assert s.ddim_alphas_prev[0] == s.ac32[0]                       # the reference's first `alphas_prev` entry is alphas_cumprod[0]
    sc = s.scale_arr[ts]
    np.testing.assert_array_equal(s.ddim_scale_arr, sc); np.testing.assert_array_equal(s.ddim_scale_arr_prev, np.concatenate([sc[:1], sc[:-1]]))
    # every step's coefficients are finite, the t = 999 one included (alpha = 0: sa = 0, sb = 1)
    for index in range(30):
        assert np.isfinite(s.step_coeffs(index)).all(), index
    assert s.step_coeffs(29)[:3] == (999, 0.0, 1.0)


def test_default_schedule_is_unchanged():
    """`make_schedule(S, eta)` without the new argument is the 'uniform' schedule of dc_schedule.npz, and naming it changes nothing"""
    from motionrag_amd.dynamicrafter import DDIMSampler
    g = np.load(os.path.join(GOLDEN, "dc_schedule.npz"))
    s, u = DDIMSampler(), DDIMSampler()
    np.testing.assert_array_equal(s.make_schedule(30, 1.0), g["t30"])
    np.testing.assert_array_equal(u.make_schedule(30, 1.0, "uniform"), g["t30"])
    for name in ("ddim_sigmas", "ddim_alphas", "ddim_alphas_prev", "ddim_scale_arr", "ddim_scale_arr_prev"):
        np.testing.assert_array_equal(getattr(s, name), getattr(u, name))
    np.testing.assert_allclose(s.ddim_sigmas, g["sigmas"], rtol=1e-6); np.testing.assert_allclose(s.ddim_alphas, g["alphas"], rtol=1e-6)
    np.testing.assert_allclose(s.ddim_alphas_prev, g["alphas_prev"], rtol=1e-6)
    np.testing.assert_array_equal(s.make_schedule(50), g["t50"])
    assert not s.ddim_sigmas.any()                                  # eta defaults to 0


@pytest.mark.parametrize("name", ["quad", "linspace", "trailing", "", None])
def test_other_spacings_raise(name):
    from motionrag_amd.dynamicrafter import DDIMSampler
    from motionrag_amd.dynamicrafter_pipeline import image_guided_synthesis
    with pytest.raises(NotImplementedError):
        DDIMSampler().make_schedule(30, 1.0, name)
    with pytest.raises(NotImplementedError):                        # refused in front of any work (no model, no device needed)
        image_guided_synthesis(None, [""], None, [1, 4, 4, 8, 8], unconditional_guidance_scale=2.0, timestep_spacing=name)


def test_sampler_refuses_a_guidance_rescale_outside_0_1():
    from motionrag_amd.dynamicrafter import DDIMSampler
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            DDIMSampler().sample(None, None, None, None, S=5, guidance_rescale=bad)


def test_rescaled_step_is_declared_and_exported():
    from motionrag_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mrag_hip.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mrag_ddim_v_rescale_workspace_bytes", "mrag_ddim_v_step_rescaled_f32"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    lib = _lib.lib()
    assert lib.mrag_abi_version() == _lib.ABI_VERSION == 11
    ws = lib.mrag_ddim_v_rescale_workspace_bytes
    assert ws(1, 2) > 0 and ws(1, 2) % 16 == 0
    assert ws(3, 589824) == 3 * ws(1, 589824) and ws(1, 589824) <= 64 * 1024     # a few partial records per sample, not a copy of it
    assert ws(1, 1 << 40) == ws(1, 1 << 30)                                       # bounded per sample
    assert ws(0, 1024) == 0 and ws(1, 1) == 0 and ws(-1, 8) == 0                  # shapes the step refuses
    # the refusals that need no device: the argument checks come before any launch
    step = lib.mrag_ddim_v_step_rescaled_f32
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(v=p, x=p, batch=1, n=8, phi=0.7, ws=p, wsb=4096)

    def call(**kw):
        a = dict(ok, **kw)
        return step(None, a["v"], a["x"], None, a["batch"], a["n"], 2.0, a["phi"], 0.5, 0.5, 1.0, 0.9, 0.1, 0.2, a["ws"], a["wsb"])

    for bad in (dict(v=None), dict(x=None), dict(ws=None), dict(batch=0), dict(n=1), dict(phi=0.0), dict(phi=-0.5), dict(phi=1.5), dict(phi=float("nan")),
                dict(wsb=ws(1, 8) - 1), dict(ws=p + 8)):
        assert call(**bad) == _lib.MRAG_EINVAL, bad
