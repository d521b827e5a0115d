"""CPU-side checks of the model's own ancestral (DDPM) sampler (audiogpt_amd/ldm/ddpm.py): its schedule buffers against the
reference-made golden (tests/golden/make_golden_ddpm.py), its method surface, its RNG consumption, which calls take the host
loop, what it hands to the device, and the argument checks of maa_ddpm_sample / maa_ddpm_update (no GPU)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd.ldm.ddpm import SCHEDULE_BUFFERS, AncestralSampling, schedule_buffers

E = inspect.Parameter.empty
SHORT8 = dict(C.LDM_T2A, timesteps=8, linear_start=0.00085 * 50, linear_end=0.0120 * 50)
# text_to_audio/Make_An_Audio/ldm/models/diffusion/ddpm_audio.py:717-905, ddpm.py:214-220 (hard-coded: the reference is not read
# at test time); p_sample_loop / progressive_denoising end with this port's private `_step_noise`
REF_SIGNATURES = {
    "predict_start_from_noise": [("self", E), ("x_t", E), ("t", E), ("noise", E)],
    "q_posterior": [("self", E), ("x_start", E), ("x_t", E), ("t", E)],
    "p_mean_variance": [("self", E), ("x", E), ("c", E), ("t", E), ("clip_denoised", E), ("return_codebook_ids", False),
                        ("quantize_denoised", False), ("return_x0", False), ("score_corrector", None), ("corrector_kwargs", None)],
    "p_sample": [("self", E), ("x", E), ("c", E), ("t", E), ("clip_denoised", False), ("repeat_noise", False),
                 ("return_codebook_ids", False), ("quantize_denoised", False), ("return_x0", False), ("temperature", 1.),
                 ("noise_dropout", 0.), ("score_corrector", None), ("corrector_kwargs", None)],
    "progressive_denoising": [("self", E), ("cond", E), ("shape", E), ("verbose", True), ("callback", None),
                              ("quantize_denoised", False), ("img_callback", None), ("mask", None), ("x0", None),
                              ("temperature", 1.), ("noise_dropout", 0.), ("score_corrector", None), ("corrector_kwargs", None),
                              ("batch_size", None), ("x_T", None), ("start_T", None), ("log_every_t", None), ("_step_noise", None)],
    "p_sample_loop": [("self", E), ("cond", E), ("shape", E), ("return_intermediates", False), ("x_T", None), ("verbose", True),
                      ("callback", None), ("timesteps", None), ("quantize_denoised", False), ("mask", None), ("x0", None),
                      ("img_callback", None), ("start_T", None), ("log_every_t", None), ("_step_noise", None)],
    "sample": [("self", E), ("cond", E), ("batch_size", 16), ("return_intermediates", False), ("x_T", None), ("verbose", True),
               ("timesteps", None), ("quantize_denoised", False), ("mask", None), ("x0", None), ("shape", None), ("kwargs", E)],
    "sample_log": [("self", E), ("cond", E), ("batch_size", E), ("ddim", E), ("ddim_steps", E), ("kwargs", E)],
}


class _RecordingUNet:
    """Stands in for backend.UNet: records what the model hands to the device loop and to the one-step update."""

    def __init__(self):
        self.loops, self.updates = [], []

    def ddpm_sample(self, x_T, tables, n, **kw):
        self.loops.append(dict(x_T=x_T, tables=tables, n=n, **kw))
        every = kw["log_every_t"]
        n_log = sum(1 for t in range(n) if t % every == 0 or t == n - 1)
        return x_T.clone(), [x_T.clone() for _ in range(n_log)], [x_T.clone() for _ in range(n_log)]

    def ddpm_update(self, x, eps, t, tables, noise, temperature=1.0, clip_denoised=True):
        self.updates.append(dict(t=t.clone(), noise=noise, temperature=temperature, clip_denoised=clip_denoised))
        return x.clone(), x.clone()


class _HostModel(AncestralSampling):
    """What the ancestral sampler reads of its model, on the CPU."""

    def __init__(self, ldm=C.LDM_T2A):
        self.device = torch.device("cpu")
        self.conditioning_key = ldm["conditioning_key"]
        self.num_timesteps = ldm["timesteps"]
        bufs = self.register_ancestral_schedule(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
        self.sqrt_alphas_cumprod = torch.from_numpy(bufs["sqrt_alphas_cumprod"])
        self.sqrt_one_minus_alphas_cumprod = torch.from_numpy(bufs["sqrt_one_minus_alphas_cumprod"])
        self.log_every_t = ldm["log_every_t"]
        self.channels, self.mel_dim, self.mel_length = ldm["latent_shape"]
        self.unet = _RecordingUNet()
        self.first_stage_model = object()          # (the KL autoencoder: no `quantize`)
        self.model_calls = 0

    def apply_model(self, x, t, c):
        self.model_calls += 1
        return torch.zeros_like(x)

    def q_sample(self, x_start, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        return x_start + noise


SHAPE = (2, 4, 10, 8)


@pytest.mark.parametrize("name", sorted(REF_SIGNATURES))
def test_methods_have_the_reference_signature(name):
    params = inspect.signature(getattr(AncestralSampling, name)).parameters
    assert [(p.name, p.default) for p in params.values()] == REF_SIGNATURES[name]


def test_model_defaults_and_config_keys():
    assert AncestralSampling.clip_denoised is True and AncestralSampling.parameterization == "eps"
    assert AncestralSampling.v_posterior == 0.0 and AncestralSampling.shorten_cond_schedule is False
    assert (C.LDM_T2A["log_every_t"], C.LDM_I2A["log_every_t"], C.LDM_INPAINT["log_every_t"]) == (200, 200, 100)
    m = _HostModel(C.LDM_INPAINT)
    assert (m.channels, m.mel_dim, m.mel_length, m.log_every_t) == (4, 10, 106, 100)
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    assert issubclass(LatentDiffusionAudio, AncestralSampling)


@pytest.mark.parametrize("tag,ldm", [("t2a", C.LDM_T2A), ("i2a", C.LDM_I2A), ("inpaint", C.LDM_INPAINT), ("short8", SHORT8)])
def test_schedule_buffers_equal_the_reference_bit_for_bit(golden, tag, ldm):
    g = golden("ddpm_schedule")
    bufs = schedule_buffers(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
    m = _HostModel(ldm)
    for name in SCHEDULE_BUFFERS:
        ref = g[tag + "_" + name]
        assert bufs[name].dtype == np.float32 and ref.dtype == np.float32
        assert bufs[name].tobytes() == ref.tobytes(), name
        assert getattr(m, name).dtype == torch.float32 and getattr(m, name).numpy().tobytes() == ref.tobytes(), name


def _reference_draws(seed, shape, n, masked, x_T_given=True):
    """The reference's draw order restated: randn(shape) for a missing x_T; per step noise_like (ddpm_audio.py:766), then
    randn_like(x0) with a mask (:874 -> ddpm.py:273)."""
    torch.manual_seed(seed)
    x_T = None if x_T_given else torch.randn(shape)
    p, q = [], []
    for _ in range(n):
        p.append(torch.randn(shape))
        if masked:
            q.append(torch.randn(shape))
    return x_T, p, q, torch.randn(16)


@pytest.mark.parametrize("masked", [False, True])
def test_seeded_p_sample_loop_draws_as_the_reference(masked):
    m = _HostModel()
    kw = dict(mask=torch.ones(SHAPE), x0=torch.zeros(SHAPE)) if masked else {}
    torch.manual_seed(11)
    m.p_sample_loop(torch.zeros(2, 4, 1024), SHAPE, timesteps=5, verbose=False, **kw)
    after = torch.randn(16)
    x_T, p, q, nxt = _reference_draws(11, SHAPE, 5, masked, x_T_given=False)
    assert torch.equal(after, nxt)
    call = m.unet.loops[-1]
    assert call["n"] == 5 and torch.equal(call["x_T"], x_T) and torch.equal(call["noise_p"], torch.stack(p))
    assert call["clip_denoised"] is True and call["log_every_t"] == 200 and call["tables"] is m
    if masked:
        assert torch.equal(call["noise_q"], torch.stack(q))
    else:
        assert "mask" not in call and "noise_q" not in call


def test_seeded_progressive_denoising_draws_as_the_reference():
    m = _HostModel()
    temps = [0.5 + 0.1 * i for i in range(6)]
    torch.manual_seed(12)
    img, logs = m.progressive_denoising(torch.zeros(4, 4, 1024), SHAPE[1:], verbose=False, batch_size=2, start_T=6,
                                        x_T=torch.zeros(SHAPE), temperature=temps, log_every_t=4)
    after = torch.randn(16)
    _, p, _, nxt = _reference_draws(12, SHAPE, 6, False)
    assert torch.equal(after, nxt)
    call = m.unet.loops[-1]
    assert call["n"] == 6 and call["temperature"] == temps and torch.equal(call["noise_p"], torch.stack(p))
    assert call["cond"].shape[0] == 2                      # the conditioning is cut to the batch (ddpm_audio.py:797-802)
    assert len(logs) == 3                                  # t = 5 (the first step run), 4, 0


@pytest.mark.parametrize("timesteps,start_T,n", [(None, None, 8), (5, None, 5), (None, 3, 3), (5, 3, 3), (3, 5, 3), (8, 100, 8)])
def test_timesteps_and_start_T_select_n_and_the_log_count(timesteps, start_T, n):
    m = _HostModel(SHORT8)
    z, inter = m.p_sample_loop(None, SHAPE, return_intermediates=True, x_T=torch.zeros(SHAPE), verbose=False, timesteps=timesteps,
                               start_T=start_T, log_every_t=2)
    assert m.unet.loops[-1]["n"] == n
    assert len(inter) == 1 + sum(1 for t in range(n) if t % 2 == 0 or t == n - 1)
    assert torch.equal(inter[0], torch.zeros(SHAPE))


class _Corrector:
    def modify_score(self, model, e_t, x, t, c):
        return e_t


HOOKS = {
    "callback": dict(callback=lambda i: None),
    "img_callback": dict(img_callback=lambda img, i: None),
    "score_corrector": dict(score_corrector=_Corrector(), corrector_kwargs={}),
    "noise_dropout": dict(noise_dropout=0.25),
}


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_each_host_hook_takes_the_host_loop(hook):
    m = _HostModel(SHORT8)
    m.progressive_denoising(None, SHAPE, verbose=False, x_T=torch.zeros(SHAPE), **HOOKS[hook])
    assert not m.unet.loops and len(m.unet.updates) == 8 and m.model_calls == 8
    assert [int(u["t"][0]) for u in m.unet.updates] == list(range(7, -1, -1))


def test_quantize_denoised_takes_the_host_loop_and_fails_as_the_reference():
    m = _HostModel(SHORT8)
    with pytest.raises(AttributeError):          # the KL first stage has no quantize (ddpm_audio.py:739)
        m.p_sample_loop(None, SHAPE, x_T=torch.zeros(SHAPE), verbose=False, quantize_denoised=True)
    assert not m.unet.loops and m.model_calls == 1


def test_nothing_else_takes_the_host_loop():
    m = _HostModel(SHORT8)
    m.progressive_denoising(None, SHAPE, verbose=False, x_T=torch.zeros(SHAPE), temperature=0.7, noise_dropout=0., start_T=4,
                            mask=torch.ones(SHAPE), x0=torch.zeros(SHAPE), corrector_kwargs=dict(a=1), log_every_t=3)
    m.sample(None, batch_size=2, x_T=torch.zeros(2, 4, 10, 78), verbose=False, timesteps=2)
    assert len(m.unet.loops) == 2 and not m.unet.updates and m.model_calls == 0
    assert m.unet.loops[1]["x_T"].shape == (2, 4, 10, 78) and m.unet.loops[1]["n"] == 2


def test_callbacks_see_i_descending_and_the_host_loop_draws_lazily_in_the_reference_order():
    m = _HostModel(SHORT8)
    seen, imgs = [], []
    torch.manual_seed(13)
    m.p_sample_loop(None, SHAPE, x_T=torch.zeros(SHAPE), verbose=False, timesteps=5, callback=seen.append,
                    img_callback=lambda img, i: imgs.append(i), mask=torch.ones(SHAPE), x0=torch.zeros(SHAPE))
    after = torch.randn(16)
    assert seen == [4, 3, 2, 1, 0] == imgs
    _, p, q, nxt = _reference_draws(13, SHAPE, 5, True)
    assert torch.equal(after, nxt)
    assert all(torch.equal(u["noise"], z) for u, z in zip(m.unet.updates, p))

    class Drawing:          # a corrector that draws: the step's noise comes after it, the dropout's mask after that
        def modify_score(self, model, e_t, x, t, c):
            return e_t + torch.randn(1)

    m = _HostModel(SHORT8)
    torch.manual_seed(14)
    m.progressive_denoising(None, SHAPE, verbose=False, x_T=torch.zeros(SHAPE), start_T=2, score_corrector=Drawing(),
                            noise_dropout=0.5)
    after = torch.randn(16)
    torch.manual_seed(14)
    for _ in range(2):
        torch.randn(1)
        torch.nn.functional.dropout(torch.randn(SHAPE) * 1.0, p=0.5)
    assert torch.equal(after, torch.randn(16))


def test_mask_without_x0_and_shortened_cond_schedule_raise():
    m = _HostModel(SHORT8)
    with pytest.raises(AssertionError):
        m.p_sample_loop(None, SHAPE, x_T=torch.zeros(SHAPE), verbose=False, mask=torch.ones(SHAPE))
    with pytest.raises(AssertionError):
        m.progressive_denoising(None, SHAPE, x_T=torch.zeros(SHAPE), verbose=False, mask=torch.ones(SHAPE))
    m.shorten_cond_schedule = True
    with pytest.raises(NotImplementedError, match="shorten_cond_schedule"):
        m.p_sample_loop(None, SHAPE, x_T=torch.zeros(SHAPE), verbose=False)
    assert not m.unet.loops


def test_sample_log_takes_both_branches():
    m = _HostModel(SHORT8)
    z, inter = m.sample_log(None, 2, False, 0, x_T=torch.zeros(2, 4, 10, 78), timesteps=3)
    assert isinstance(inter, list) and torch.equal(inter[0], torch.zeros(2, 4, 10, 78)) and m.unet.loops[-1]["n"] == 3
    seen = {}

    class U(_RecordingUNet):
        def ddim_sample(self, x_T, timesteps, alphas, alphas_prev, **kw):
            seen["S"] = len(timesteps)
            return x_T.clone(), [], []

    m = _HostModel()
    m.unet = U()
    m.alphas_cumprod = torch.from_numpy(schedule_buffers(1000, 0.00085, 0.012)["alphas_cumprod"])
    z, inter = m.sample_log(None, 2, True, 10, x_T=torch.zeros(2, 4, 10, 78))
    assert seen["S"] == 10 and set(inter) == {"x_inter", "pred_x0"}


def test_unknown_sampler_names_all_three():
    from audiogpt_amd._lib import MaaError
    from audiogpt_amd.pipeline import MakeAnAudio
    with pytest.raises(MaaError, match=r'"ddim", "plms" or "ddpm".*bogus'):
        MakeAnAudio.sample_latents(object(), torch.zeros(1, 4, 10, 8), sampler="bogus")


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _fake(n=1):
    return ctypes.c_void_p(16 * n)          # a non-null pointer that the argument checks never dereference


def test_exports_hold_the_two_new_entries():
    from audiogpt_amd import _lib
    assert "maa_ddpm_sample" in _lib.EXPORTS and "maa_ddpm_update" in _lib.EXPORTS


def test_ddpm_sample_entry_rejects_bad_arguments(lib):
    from audiogpt_amd import _lib
    T = 8
    tab = np.linspace(0.1, 0.9, T).astype(np.float32)
    fp = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    a = _lib.maa_ddpm_args()
    a.loop.S, a.loop.B, a.loop.C, a.loop.H, a.loop.W, a.loop.scale = T, 1, 4, 10, 8, 1.0
    a.start, a.n, a.clip_denoised = T - 1, T, 1
    a.h_sqrt_recip_ac = a.h_sqrt_recipm1_ac = a.h_coef1 = a.h_coef2 = a.h_logvar = fp
    a.loop.d_noise_p = 16

    def fails(msg):
        assert lib.maa_ddpm_sample(None, _fake(), ctypes.byref(a), _fake()) < 0
        assert msg in lib.maa_last_error(), lib.maa_last_error()

    assert lib.maa_ddpm_sample(None, None, None, None) < 0
    assert b"bad ddpm_sample" in lib.maa_last_error()
    fails(b"null context")          # well-formed arguments reach the context, which is null here
    a.loop.B = 0
    fails(b"empty problem")
    a.loop.B = 1
    for n, start in ((0, T - 1), (T + 1, T - 1)):
        a.n, a.start = n, start
        fails(b"1 .. num_timesteps")
    a.n, a.start = 4, 2
    fails(b"outside the schedule")
    a.n, a.start = 4, T
    fails(b"outside the schedule")
    a.n, a.start = T, T - 1
    a.h_logvar = None
    fails(b"posterior tables")
    a.h_logvar = fp
    a.loop.d_noise_p = None
    fails(b"noise is missing")
    a.loop.d_noise_p = 16
    a.loop.d_mask = 16
    fails(b"mask needs x0")
    a.loop.d_x0 = 16
    fails(b"mask needs x0")
    a.loop.d_noise_q = 16
    fails(b"mask needs x0")          # ... and the q_sample tables
    a.h_sqrt_ac = a.h_sqrt_1mac = fp
    fails(b"null context")
    a.loop.d_mask = a.loop.d_x0 = a.loop.d_noise_q = None
    a.loop.log_every_t, a.loop.n_log, a.loop.d_log_x, a.loop.d_log_x0 = 2, 4, 16, 16          # t = 7, 6, 4, 2, 0: five
    fails(b"n_log does not match")
    a.loop.n_log = 5
    fails(b"null context")
    a.n, a.start = 4, 7                                     # t = 7, 6, 5, 4: three
    fails(b"n_log does not match")
    a.loop.n_log = 3
    fails(b"null context")
    a.loop.d_log_x0 = None
    fails(b"intermediates need their buffers")


def test_ddpm_update_entry_rejects_bad_arguments(lib):
    tab = np.linspace(0.1, 0.9, 8).astype(np.float32)
    fp = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ok = [None, _fake(1), _fake(2), _fake(3), fp, fp, fp, fp, fp, 8, _fake(4), 1.0, 1, 1, 4, 10, 8, _fake(5), _fake(6)]
    assert lib.maa_ddpm_update(*ok) < 0 and b"null context" in lib.maa_last_error()
    for i, v, msg in ((1, None, b"null pointer"), (8, None, b"posterior tables"), (9, 0, b"empty"), (13, 0, b"empty"),
                      (17, _fake(1), b"alias")):
        bad = list(ok)
        bad[i] = v
        assert lib.maa_ddpm_update(*bad) < 0 and msg in lib.maa_last_error(), (i, lib.maa_last_error())
