"""CPU-side checks of PLMS sampling: PLMSSampler's surface, its schedule tables against the reference-made goldens
(tests/golden/make_golden_plms.py), its RNG consumption and what it hands to the device, and the argument checks of
maa_ldm_plms_sample (no GPU)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd.pipeline import alphas_cumprod_f32

E = inspect.Parameter.empty
# text_to_audio/Make_An_Audio/ldm/models/diffusion/plms.py:12, 24, 58-80 (hard-coded: the reference is not read at test time)
REF_SIGNATURES = {
    "__init__": [("self", E), ("model", E), ("schedule", "linear"), ("kwargs", E)],
    "make_schedule": [("self", E), ("ddim_num_steps", E), ("ddim_discretize", "uniform"), ("ddim_eta", 0.0), ("verbose", True)],
    "sample": [("self", E), ("S", E), ("batch_size", E), ("shape", E), ("conditioning", None), ("callback", None),
               ("normals_sequence", None), ("img_callback", None), ("quantize_x0", False), ("eta", 0.0), ("mask", None),
               ("x0", None), ("temperature", 1.0), ("noise_dropout", 0.0), ("score_corrector", None),
               ("corrector_kwargs", None), ("verbose", True), ("x_T", None), ("log_every_t", 100),
               ("unconditional_guidance_scale", 1.0), ("unconditional_conditioning", None), ("kwargs", E)],
}


class _RecordingUNet:
    """Stands in for backend.UNet: records what the sampler hands to the device loop."""

    def __init__(self):
        self.calls = []

    def plms_sample(self, x_T, timesteps, alphas, alphas_prev, **kw):
        self.calls.append(dict(x_T=x_T, timesteps=np.asarray(timesteps), alphas=np.asarray(alphas),
                               alphas_prev=np.asarray(alphas_prev), **kw))
        return x_T.clone(), [], []


class _HostModel:
    """What PLMSSampler reads of its model: the schedule, the q_sample buffers, the conditioning key and the device."""

    def __init__(self):
        ldm = C.LDM_T2A
        ac = alphas_cumprod_f32(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
        self.num_timesteps = ldm["timesteps"]
        self.alphas_cumprod = torch.from_numpy(ac)
        self.sqrt_alphas_cumprod = torch.from_numpy(np.sqrt(ac))
        self.sqrt_one_minus_alphas_cumprod = torch.from_numpy(np.sqrt(np.float32(1.0) - ac))
        self.device = torch.device("cpu")
        self.conditioning_key = "crossattn"
        self.unet = _RecordingUNet()


def _sampler():
    from audiogpt_amd.ldm.plms import PLMSSampler
    return PLMSSampler(_HostModel())


def _t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.mark.parametrize("name", sorted(REF_SIGNATURES))
def test_plms_sampler_has_the_reference_signature(name):
    from audiogpt_amd.ldm.plms import PLMSSampler
    params = inspect.signature(getattr(PLMSSampler, name)).parameters
    assert [(p.name, p.default) for p in params.values()] == REF_SIGNATURES[name]


def test_plms_needs_eta_zero():
    s = _sampler()
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        s.make_schedule(10, ddim_eta=0.5, verbose=False)
    with pytest.raises(ValueError, match="ddim_eta must be 0 for PLMS"):
        s.sample(10, 1, [4, 10, 78], eta=0.1, verbose=False)
    with pytest.raises(NotImplementedError):
        s.make_schedule(10, ddim_discretize="quad", verbose=False)


@pytest.mark.parametrize("name", ["plms_t2a_s10", "plms_t2a_mask_s6"])
def test_schedule_tables_equal_the_reference(golden, name):
    g = golden(name)
    s = _sampler()
    s.make_schedule(int(g["S"]), verbose=False)
    np.testing.assert_array_equal(np.asarray(s.ddim_timesteps), g["ddim_timesteps"])
    np.testing.assert_array_equal(s.ddim_alphas.numpy(), g["ddim_alphas"])
    np.testing.assert_array_equal(np.asarray(s.ddim_alphas_prev, dtype=np.float32), g["ddim_alphas_prev"])
    np.testing.assert_array_equal(s.ddim_sqrt_one_minus_alphas.numpy(), g["ddim_sqrt_one_minus_alphas"])
    assert np.all(np.asarray(s.ddim_sigmas) == 0.0)


def test_single_and_five_step_schedules_match_the_reference(golden):
    g = golden("plms_t2a_orders")
    for S in (1, 5):
        s = _sampler()
        s.make_schedule(S, verbose=False)
        np.testing.assert_array_equal(np.asarray(s.ddim_timesteps), g[f"ddim_timesteps_s{S}"])


def test_seeded_sample_draws_as_the_reference(golden):
    g = golden("plms_t2a_s10")
    s = _sampler()
    torch.manual_seed(int(g["seed"]))
    s.sample(int(g["S"]), 2, list(g["x_T"].shape[1:]), conditioning=_t(g["c"]), verbose=False, x_T=_t(g["x_T"]),
             log_every_t=int(g["log_every_t"]), unconditional_guidance_scale=float(g["scale"]), unconditional_conditioning=_t(g["uc"]))
    assert torch.equal(torch.randn(g["next_draw"].shape[0]), _t(g["next_draw"]))
    call = s.model.unet.calls[-1]
    assert "mask" not in call
    assert call["log_every_t"] == int(g["log_every_t"]) and call["scale"] == float(g["scale"])
    np.testing.assert_array_equal(call["timesteps"], g["ddim_timesteps"])
    np.testing.assert_array_equal(call["alphas"], g["ddim_alphas"])
    assert "sigmas" not in call and "noise_p" not in call


def test_seeded_masked_sample_draws_as_the_reference_and_hands_over_its_q_noise(golden):
    g = golden("plms_t2a_mask_s6")
    s = _sampler()
    torch.manual_seed(int(g["seed"]))
    s.sample(int(g["S"]), 2, list(g["x_T"].shape[1:]), conditioning=_t(g["c"]), verbose=False, x_T=_t(g["x_T"]), mask=_t(g["mask"]),
             x0=_t(g["x0"]), log_every_t=int(g["log_every_t"]), unconditional_guidance_scale=float(g["scale"]),
             unconditional_conditioning=_t(g["uc"]))
    assert torch.equal(torch.randn(g["next_draw"].shape[0]), _t(g["next_draw"]))
    call = s.model.unet.calls[-1]
    assert len(g["ddim_timesteps"]) == 7
    assert torch.equal(call["noise_q"], _t(g["noise_q"]))
    np.testing.assert_array_equal(call["sqrt_ac"], s.model.sqrt_alphas_cumprod.numpy()[g["ddim_timesteps"]])


def test_unseeded_x_T_is_drawn_first():
    """x_T=None: the first draw is x_T itself (plms.py:128-129), then the loop's; two draws at step 0, one after."""
    s = _sampler()
    torch.manual_seed(7)
    s.sample(4, 1, [4, 10, 8], verbose=False)
    after = torch.randn(4)
    torch.manual_seed(7)
    x_T = torch.randn(1, 4, 10, 8)
    for _ in range(4 + 1):
        torch.randn(1, 4, 10, 8)
    assert torch.equal(after, torch.randn(4))
    assert torch.equal(s.model.unet.calls[-1]["x_T"], x_T)


def test_masked_sample_needs_x0():
    s = _sampler()
    with pytest.raises(AssertionError):
        s.sample(4, 1, [4, 10, 8], verbose=False, mask=torch.ones(1, 1, 10, 8))


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _fake(n=1):
    return ctypes.c_void_p(16 * n)          # a non-null pointer that the argument checks never dereference


def test_ldm_plms_entry_rejects_bad_arguments(lib):
    from audiogpt_amd import _lib
    S = 10
    ts = np.arange(1, 1000, 100).astype(np.int32)
    al = np.linspace(0.99, 0.01, S).astype(np.float32)
    a = _lib.maa_ddim_args()
    a.S, a.B, a.C, a.H, a.W, a.scale = S, 1, 4, 10, 78, 1.0
    a.h_timesteps = ts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    a.h_alphas = a.h_alphas_prev = al.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.maa_ldm_plms_sample(None, None, None, None) < 0
    assert b"bad" in lib.maa_last_error()
    assert lib.maa_ldm_plms_sample(None, _fake(), ctypes.byref(a), None) < 0
    assert b"bad" in lib.maa_last_error()
    a.h_sigmas = al.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.maa_ldm_plms_sample(None, _fake(), ctypes.byref(a), _fake()) < 0
    assert b"ddim_eta must be 0" in lib.maa_last_error()
    a.h_sigmas = None
    a.d_noise_p = 16
    assert lib.maa_ldm_plms_sample(None, _fake(), ctypes.byref(a), _fake()) < 0
    assert b"ddim_eta must be 0" in lib.maa_last_error()
    a.d_noise_p = None
    a.S = 0
    assert lib.maa_ldm_plms_sample(None, _fake(), ctypes.byref(a), _fake()) < 0
    assert b"empty" in lib.maa_last_error()
    a.S = S
    # well-formed arguments reach the context, which is null here
    assert lib.maa_ldm_plms_sample(None, _fake(), ctypes.byref(a), _fake()) < 0
    assert b"null context" in lib.maa_last_error()
