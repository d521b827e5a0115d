"""CPU-side checks of text-guided editing (SDEdit): DDIMSampler.stochastic_encode / decode's surface, the sampler's new
tables, the golden files' own arithmetic and the argument checks of maa_ddim_stochastic_encode / maa_ddim_decode (no GPU)."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd.pipeline import alphas_cumprod_f32

# text_to_audio/Make_An_Audio/ldm/models/diffusion/ddim.py:227, 243-244 (hard-coded: the reference is not read at test time)
REF_SIGNATURES = {
    "stochastic_encode": [("self", inspect.Parameter.empty), ("x0", inspect.Parameter.empty), ("t", inspect.Parameter.empty),
                          ("use_original_steps", False), ("noise", None)],
    "decode": [("self", inspect.Parameter.empty), ("x_latent", inspect.Parameter.empty), ("cond", inspect.Parameter.empty),
               ("t_start", inspect.Parameter.empty), ("unconditional_guidance_scale", 1.0),
               ("unconditional_conditioning", None), ("use_original_steps", False)],
}


class _HostModel:
    """What DDIMSampler reads of its model before any device work: the schedule and the device."""

    def __init__(self):
        ldm = C.LDM_T2A
        self.num_timesteps = ldm["timesteps"]
        self.alphas_cumprod = torch.from_numpy(alphas_cumprod_f32(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"]))
        self.device = torch.device("cpu")
        self.conditioning_key = "crossattn"


def _sampler():
    from audiogpt_amd.ldm.ddim import DDIMSampler
    return DDIMSampler(_HostModel())


@pytest.mark.parametrize("name", sorted(REF_SIGNATURES))
def test_sdedit_methods_have_the_reference_signature(name):
    from audiogpt_amd.ldm.ddim import DDIMSampler
    params = inspect.signature(getattr(DDIMSampler, name)).parameters
    assert [(p.name, p.default) for p in params.values()] == REF_SIGNATURES[name]


def test_sampler_q_sample_tables_are_the_fp32_restatement(golden):
    s = _sampler()
    s.make_schedule(10, verbose=False)
    ac = alphas_cumprod_f32(1000, C.LDM_T2A["linear_start"], C.LDM_T2A["linear_end"])
    assert s.sqrt_alphas_cumprod.dtype == torch.float32 and s.sqrt_one_minus_alphas_cumprod.dtype == torch.float32
    np.testing.assert_array_equal(s.sqrt_alphas_cumprod.numpy(), np.sqrt(ac))
    np.testing.assert_array_equal(s.sqrt_one_minus_alphas_cumprod.numpy(), np.sqrt(np.float32(1.0) - ac))
    # and the reference sampler's own buffers (tests/golden/make_golden_sdedit.py), bit for bit
    g = golden("sdedit_encode")
    np.testing.assert_array_equal(s.sqrt_alphas_cumprod.numpy(), g["sqrt_ac"])
    np.testing.assert_array_equal(s.sqrt_one_minus_alphas_cumprod.numpy(), g["sqrt_1mac"])
    np.testing.assert_array_equal(torch.sqrt(s.ddim_alphas).numpy(), g["sqrt_a"])
    np.testing.assert_array_equal(s.ddim_sqrt_one_minus_alphas.numpy(), g["sqrt_1ma"])


def test_sdedit_encode_golden_is_self_consistent(golden):
    g = golden("sdedit_encode")
    x0, noise = torch.from_numpy(g["x0"]), torch.from_numpy(g["noise"])
    for t, a, b, out in ((g["t"], g["sqrt_a"], g["sqrt_1ma"], g["out"]), (g["t_orig"], g["sqrt_ac"], g["sqrt_1mac"], g["out_orig"])):
        assert len(set(t.tolist())) == 3
        ta, tb = torch.from_numpy(a)[torch.from_numpy(t)], torch.from_numpy(b)[torch.from_numpy(t)]
        ref = ta.view(-1, 1, 1, 1) * x0 + tb.view(-1, 1, 1, 1) * noise
        assert torch.equal(ref, torch.from_numpy(out))


def test_sdedit_chain_golden_is_self_consistent(golden):
    g = golden("sdedit_chain")
    t_enc = int(g["t_enc"])
    assert t_enc == int(float(g["strength"]) * int(g["S"]))
    ac = alphas_cumprod_f32(1000, C.LDM_T2A["linear_start"], C.LDM_T2A["linear_end"])
    steps = np.asarray(list(range(0, 1000, 1000 // int(g["S"])))) + 1
    a = torch.from_numpy(ac[steps])
    ref = torch.sqrt(a)[t_enc] * torch.from_numpy(g["z0"]) + torch.sqrt(1.0 - a)[t_enc] * torch.from_numpy(g["n_q"])
    assert torch.equal(ref, torch.from_numpy(g["z_enc"]))
    T = g["mel_in"].shape[-1]
    assert g["mel_in"].shape == (2, 1, 80, T) and g["spec"].shape == (2, 80, T) and g["wav"].shape == (2, T * 256)
    assert g["z_enc"].shape == (2, 4, 10, T // 8)


def test_sdedit_methods_need_a_schedule_as_in_the_reference():
    s = _sampler()
    x = torch.zeros(1, 4, 10, 78)
    with pytest.raises(AttributeError):
        s.stochastic_encode(x, torch.tensor([0]))
    with pytest.raises(AttributeError):
        s.stochastic_encode(x, torch.tensor([0]), use_original_steps=True)
    with pytest.raises(AttributeError):
        s.decode(x, None, 3)


def test_decode_over_the_ddpm_steps_fails_as_in_the_reference():
    s = _sampler()
    s.make_schedule(10, verbose=False)
    x = torch.zeros(1, 4, 10, 78)
    with pytest.raises(AttributeError, match="ddim_sigmas_for_original_num_steps"):
        s.decode(x, None, 5, use_original_steps=True)
    assert s.decode(x, None, 0, use_original_steps=True) is x      # the reference's loop is empty: nothing is read
    assert s.decode(x, None, 0) is x


def test_stochastic_encode_checks_t_on_the_host():
    from audiogpt_amd import _lib
    from audiogpt_amd.backend import ddim_stochastic_encode
    ctx = types.SimpleNamespace(device=torch.device("cpu"))       # every check below fails before the library is reached
    x, tab = torch.zeros(2, 4, 10, 78), np.ones(10, np.float32)
    with pytest.raises(_lib.MaaError, match="t must lie"):
        ddim_stochastic_encode(ctx, x, torch.tensor([0, 10]), tab, tab, x)
    with pytest.raises(_lib.MaaError, match="t must lie"):
        ddim_stochastic_encode(ctx, x, -1, tab, tab, x)
    with pytest.raises(_lib.MaaError, match="one integer index per sample"):
        ddim_stochastic_encode(ctx, x, torch.tensor([0, 1, 2]), tab, tab, x)
    with pytest.raises(_lib.MaaError, match="noise must be"):
        ddim_stochastic_encode(ctx, x, 3, tab, tab, x[:1])
    with pytest.raises(_lib.MaaError, match="moments"):
        ddim_stochastic_encode(ctx, x, 3, tab, tab, x[:, :2], moments=True)


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _fake(n=1):
    return ctypes.c_void_p(16 * n)          # a non-null pointer that the argument checks never dereference


def test_stochastic_encode_entry_rejects_bad_arguments(lib):
    fp = ctypes.POINTER(ctypes.c_float)
    tab = (ctypes.c_float * 10)()
    h = ctypes.cast(tab, fp)
    assert lib.maa_ddim_stochastic_encode(None, None, 0, 1.0, None, None, None, None, 10, None, 1, 4, 10, 78, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_ddim_stochastic_encode(None, _fake(), 0, 1.0, None, _fake(), h, h, 0, _fake(), 1, 4, 10, 78, _fake()) < 0
    assert b"empty" in lib.maa_last_error()
    assert lib.maa_ddim_stochastic_encode(None, _fake(), 0, 1.0, None, _fake(), h, h, 10, _fake(), 0, 4, 10, 78, _fake()) < 0
    assert b"empty" in lib.maa_last_error()
    assert lib.maa_ddim_stochastic_encode(None, _fake(), 1, 1.0, None, _fake(), h, h, 10, _fake(), 1, 4, 10, 78, _fake()) < 0
    assert b"posterior noise" in lib.maa_last_error()
    # well-formed arguments reach the context, which is null here
    assert lib.maa_ddim_stochastic_encode(None, _fake(), 0, 1.0, None, _fake(), h, h, 10, _fake(), 1, 4, 10, 78, _fake()) < 0
    assert b"null context" in lib.maa_last_error()


def test_decode_entry_rejects_bad_arguments(lib):
    from audiogpt_amd import _lib
    S = 10
    ts = np.arange(1, 1000, 100).astype(np.int32)
    al = np.linspace(0.99, 0.01, S).astype(np.float32)
    a = _lib.maa_ddim_args()
    a.S, a.B, a.C, a.H, a.W, a.scale = S, 1, 4, 10, 78, 1.0
    a.h_timesteps = ts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    a.h_alphas = a.h_alphas_prev = al.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.maa_ddim_decode(None, None, None, 1, None) < 0
    assert b"bad" in lib.maa_last_error()
    assert lib.maa_ddim_decode(None, _fake(), ctypes.byref(a), S + 1, _fake()) < 0
    assert b"t_start" in lib.maa_last_error()
    assert lib.maa_ddim_decode(None, _fake(), ctypes.byref(a), -1, _fake()) < 0
    assert b"t_start" in lib.maa_last_error()
    a.d_mask = 16
    assert lib.maa_ddim_decode(None, _fake(), ctypes.byref(a), 3, _fake()) < 0
    assert b"mask" in lib.maa_last_error()
    a.d_mask = None
    a.n_log = 2
    assert lib.maa_ddim_decode(None, _fake(), ctypes.byref(a), 3, _fake()) < 0
    assert b"intermediates" in lib.maa_last_error()
    a.n_log = 0
    assert lib.maa_ddim_decode(None, _fake(), ctypes.byref(a), S, _fake()) < 0
    assert b"null context" in lib.maa_last_error()
