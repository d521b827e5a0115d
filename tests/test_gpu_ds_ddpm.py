"""DiffSinger's ancestral sampling branch on the device: ds_ddpm_step_kernel / ds_ddpm_update_kernel (csrc/sampler_steps.hip),
DiffNet::ddpm_sample (csrc/diffnet.cpp), and GaussianDiffusion.p_sample / sample_ddpm / infer, OfflineGaussianDiffusion
(audiogpt_amd/diffsinger.py).

Goldens: tests/golden/ds_ddpm_*.npz, written by tests/golden/make_golden_ds_ddpm.py from the reference's own GaussianDiffusion
(shallow_diffusion_tts.py) on the CPU with every draw recorded.  Gates are the ones this denoiser already has in
tests/test_gpu_diffsinger.py: tol = 1e-4 (f32) / 2e-4 (bf16x3) for one denoiser evaluation, 5 * tol for a trajectory of at most 8
steps.  The reference's own fp32 rounding over these chains, measured by the same script against a float64 run, is 3.2e-7 (clip on),
9.7e-7 (clip off), 4.2e-7 (cosine), 2.7e-7 (33 frames): more than 300 times below the gates.
"""
import ctypes

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests.util import check

pytestmark = pytest.mark.gpu

PRECISIONS = [("f32", 1e-4), ("bf16x3", 2e-4)]
DIL4 = C.DIFFSINGER_DS100_ADJ_REL      # timesteps 100, max_beta 0.06, dilation cycle 4: the denoiser of DIFFSINGER_DS1000 as well
DIL1 = C.DIFFSINGER_POPCS_BETA6        # dilation cycle 1


class Rig:
    """One context and one denoiser per (precision, dilation cycle), shared by the tests of this file."""

    def __init__(self):
        self.made = {}

    def __call__(self, precision, cfg):
        from audiogpt_amd.backend import Context, DiffNet
        key = (precision, cfg["dilation_cycle_length"])
        if key not in self.made:
            ctx = Context("cuda:0", precision=precision)
            self.made[key] = (ctx, DiffNet(ctx, cfg, WT.make_diffnet_state_dict(cfg, seed=7)))
        return self.made[key]

    def close(self):
        for ctx, net in self.made.values():
            net.close()
            ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def tables(cfg, betas=None):
    """The step's five host tables from the schedule alone (no device needed)."""
    from audiogpt_amd.diffsinger import schedule_buffers
    b = schedule_buffers(cfg["timesteps"], cfg.get("schedule_type"), cfg.get("max_beta", 0.01), betas)
    sigma = (0.5 * torch.from_numpy(b["posterior_log_variance_clipped"])).exp().numpy()
    return (b["sqrt_recip_alphas_cumprod"], b["sqrt_recipm1_alphas_cumprod"], b["posterior_mean_coef1"], b["posterior_mean_coef2"], sigma)


def case(golden, name, prefix=""):
    g = golden(name)
    get = lambda k: torch.from_numpy(g[prefix + k])    # noqa: E731
    return get, int(g[prefix + "K_step"])


CHAINS = [("b2_k8", "ds_ddpm_b2_k8", "", DIL4, True, "x_inter"), ("b2_k8_noclip", "ds_ddpm_b2_k8", "", DIL4, False, "x_inter_noclip"),
          ("cosine_k8", "ds_ddpm_cosine_k8", "", dict(DIL4, schedule_type=None), True, "x_inter"),
          ("ragged_b3_t33", "ds_ddpm_ragged", "t33.", DIL1, True, "x_inter"), ("ragged_t1", "ds_ddpm_ragged", "t1.", DIL1, True, "x_inter")]


@pytest.mark.parametrize("precision,tol", PRECISIONS)
@pytest.mark.parametrize("tag,name,prefix,cfg,clip,key", CHAINS, ids=[c[0] for c in CHAINS])
def test_chain_matches_reference(golden, rig, precision, tol, tag, name, prefix, cfg, clip, key):
    """The device loop against the reference's final x; every intermediate against the reference's through the device p_sample
    arithmetic driven step by step from Python (denoiser, then maa_ds_ddpm_update) -- which must equal the loop bit for bit."""
    get, K = case(golden, name, prefix)
    ctx, net = rig(precision, cfg)
    tabs = tables(cfg)
    cond, x_T, noise, ref = get("cond"), get("x_T"), get("noise"), get(key)
    B = x_T.shape[0]
    eps0 = net(x_T, torch.full((B,), K - 1), cond)
    check(f"{precision}_ds_ddpm_{tag}_eps0", eps0, get("eps0"), tol)
    x0 = net.ddpm_sample(x_T, cond, tabs, K - 1, K, noise, clip_denoised=clip)
    check(f"{precision}_ds_ddpm_{tag}_x0", x0, ref[-1], 5 * tol)
    x = x_T.cuda()
    for k in range(K):
        t = torch.full((B,), K - 1 - k)
        x = net.ddpm_update(x, net(x, t, cond), t, tabs, noise[k], clip_denoised=clip)
        check(f"{precision}_ds_ddpm_{tag}_step{k}", x, ref[k], 5 * tol)
    assert torch.equal(x, x0), "the device loop differs from p_sample driven step by step"


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_loop_identities(golden, rig, precision, tol):
    get, K = case(golden, "ds_ddpm_b2_k8")
    ctx, net = rig(precision, DIL4)
    tabs = tables(DIL4)
    cond, x_T, noise = get("cond").cuda(), get("x_T").cuda(), get("noise").cuda()
    x0 = net.ddpm_sample(x_T, cond, tabs, K - 1, K, noise)
    assert torch.equal(x_T, get("x_T").cuda()), "the caller's x was written"
    assert torch.equal(net.ddpm_sample(x_T, cond, tabs, K - 1, K, noise, use_graph=False), x0), "graph replay differs from the eager loop"
    assert torch.equal(net.ddpm_sample(x_T, cond, tabs, K - 1, K, noise), x0), "a second call differs"
    # a chain equals its consecutive parts: 8 = 5 + 3 (what lets sample_ddpm bound the noise buffer), and 8 = 1 * 8
    part = net.ddpm_sample(x_T, cond, tabs, K - 1, 5, noise[:5])
    assert torch.equal(net.ddpm_sample(part, cond, tabs, K - 6, 3, noise[5:]), x0)
    x = x_T
    for k in range(K):
        x = net.ddpm_sample(x, cond, tabs, K - 1 - k, 1, noise[k:k + 1], use_graph=bool(k % 2))
    assert torch.equal(x, x0)
    # rows are independent
    for b in range(2):
        assert torch.equal(net.ddpm_sample(x_T[b:b + 1], cond[b:b + 1], tabs, K - 1, K, noise[:, b:b + 1].contiguous()), x0[b:b + 1])
    # the two loops share the denoiser's loop state: a PLMS call in between changes neither
    gp = golden("diffsinger_ds1000")
    pc, px = torch.from_numpy(gp["cond"]), torch.from_numpy(gp["x_T"])
    plms = lambda: net.plms_sample(px, pc, gp["alphas_cumprod"], int(gp["K_step"]), C.DIFFSINGER_DS1000["pndm_speedup"])    # noqa: E731
    p0 = plms()
    check(f"{precision}_plms_x0_after_ancestral_call", p0, gp["x0"], 5 * tol)
    assert torch.equal(net.ddpm_sample(x_T, cond, tabs, K - 1, K, noise), x0), "a PLMS call changed the ancestral chain"
    assert torch.equal(plms(), p0), "an ancestral call changed the PLMS result"


def test_plms_result_is_unchanged_by_an_ancestral_call_before_it(golden):
    """On a fresh denoiser: PLMS alone, then on another fresh one an ancestral call first (f32; the shared rig is not used)."""
    from audiogpt_amd.backend import Context, DiffNet
    gp = golden("diffsinger_ds1000")
    get, K = case(golden, "ds_ddpm_cosine_k8")
    cfg = C.DIFFSINGER_DS1000
    pc, px = torch.from_numpy(gp["cond"]), torch.from_numpy(gp["x_T"])
    out = []
    for first in (False, True):
        ctx = Context("cuda:0", precision="f32")
        net = DiffNet(ctx, cfg, WT.make_diffnet_state_dict(cfg, seed=7))
        if first:
            net.ddpm_sample(get("x_T"), get("cond"), tables(DIL4), K - 1, K, get("noise"))
        out.append(net.plms_sample(px, pc, gp["alphas_cumprod"], int(gp["K_step"]), cfg["pndm_speedup"]))
        net.close()
        ctx.close()
    assert torch.equal(out[0], out[1])
    check("f32_plms_x0_vs_reference_after_ancestral", out[1], gp["x0"], 5e-4)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_infer_matches_the_references_forward(golden, rig, precision, tol):
    """GaussianDiffusion.infer / OfflineGaussianDiffusion.infer against the reference's forward(infer=True) through its fs2 stub,
    on the draws it made (q_sample's, the gaussian start, one per step), in its order."""
    from audiogpt_amd.diffsinger import GaussianDiffusion, OfflineGaussianDiffusion
    g = golden("ds_ddpm_forward_infer")
    K = int(g["K_step"])
    ctx, net = rig(precision, DIL1)
    fs2, cond = torch.from_numpy(g["fs2_mel"]), torch.from_numpy(g["decoder_inp"]).transpose(1, 2).contiguous().cuda()
    mel2ph = torch.from_numpy(g["mel2ph"])
    for tag, cls, gs, m2p in (("plain", GaussianDiffusion, False, None), ("gstart", GaussianDiffusion, True, None),
                              ("mel2ph", GaussianDiffusion, False, mel2ph), ("offline", OfflineGaussianDiffusion, False, mel2ph)):
        gd = cls(dict(DIL1, K_step=K, gaussian_start=gs), ctx=ctx, denoise_fn=net)
        d = torch.from_numpy(g[tag + ".draws"]).cuda()
        assert d.shape[0] == 1 + int(gs) + K
        mel = gd.infer(fs2, cond, noise=d[0], noise_start=d[1] if gs else None, noise_p=d[1 + int(gs):], mel2ph=m2p)
        check(f"{precision}_ds_ddpm_infer_{tag}", mel, g[tag + ".mel_out"], 5 * tol)
        if tag == "mel2ph":
            assert bool((mel.cpu()[mel2ph == 0] == 0).all())
        # small caps cut the chain into parts: the same result, bit for bit
        per = d[0].numel() * 4
        parts = gd.denorm_spec(gd.sample_ddpm(d[1] if gs else gd.q_sample(gd.norm_spec(fs2.cuda()).transpose(1, 2)[:, None],
                                                                        torch.tensor([K - 1], device="cuda"), d[0]),
                                              cond, noise_p=d[1 + int(gs):], noise_cap_bytes=3 * per)[:, 0].transpose(1, 2))
        if m2p is not None and cls is GaussianDiffusion:
            parts = parts * (m2p.cuda() > 0).float()[:, :, None]
        assert torch.equal(parts, mel), tag


def test_infer_seeded_consumes_the_generator_as_the_reference_does(golden, rig):
    from audiogpt_amd.diffsinger import GaussianDiffusion
    g = golden("ds_ddpm_forward_infer")
    K = int(g["K_step"])
    ctx, net = rig("f32", DIL1)
    fs2, cond = torch.from_numpy(g["fs2_mel"]), torch.from_numpy(g["decoder_inp"]).transpose(1, 2).contiguous().cuda()
    for gs in (False, True):
        gd = GaussianDiffusion(dict(DIL1, K_step=K, gaussian_start=gs), ctx=ctx, denoise_fn=net)
        torch.manual_seed(123)
        mel = gd.infer(fs2, cond)
        state = torch.cuda.get_rng_state()
        # the same draws by hand, fed back in: same state after, same result
        x0 = gd.norm_spec(fs2.cuda()).transpose(1, 2)[:, None]
        torch.manual_seed(123)
        q = torch.randn_like(x0)
        start = torch.randn(x0.shape, device="cuda") if gs else None
        steps = torch.stack([torch.randn(x0.shape, device="cuda") for _ in range(K)])
        assert torch.equal(torch.cuda.get_rng_state(), state)
        assert torch.equal(gd.infer(fs2, cond, noise=q, noise_start=start, noise_p=steps), mel)
        # the cap does not change what is drawn
        torch.manual_seed(123)
        q2 = torch.randn_like(x0)
        x = torch.randn(x0.shape, device="cuda") if gs else gd.q_sample(x0, torch.tensor([K - 1], device="cuda"), q2)
        cut = gd.sample_ddpm(x, cond, noise_cap_bytes=3 * x0.numel() * 4)
        assert torch.equal(torch.cuda.get_rng_state(), state)
        assert torch.equal(gd.denorm_spec(cut[:, 0].transpose(1, 2)), mel)


@pytest.mark.parametrize("precision,tol", PRECISIONS)
def test_p_sample_with_a_timestep_per_sample(golden, rig, precision, tol):
    """p_sample / p_mean_variance with t = [0, 37, 99]: one denoiser evaluation, so the one-evaluation gate."""
    from audiogpt_amd.diffsinger import GaussianDiffusion
    g = golden("ds_ddpm_p_sample_t")
    ctx, net = rig(precision, DIL1)
    gd = GaussianDiffusion(DIL1, ctx=ctx, denoise_fn=net)
    x, cond, t = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["cond"]).cuda(), torch.from_numpy(g["t"])
    B = x.shape[0]
    eps = net(x, t, cond)
    for tag in ("each", "repeat"):
        z = torch.from_numpy(g[tag + ".noise"]).expand(B, -1, -1, -1).contiguous()
        check(f"{precision}_ds_ddpm_p_sample_t_{tag}", net.ddpm_update(x, eps, t, gd._ddpm_tables, z), g[tag + ".out"], tol)
    mean, var, logvar = gd.p_mean_variance(x, t, cond, clip_denoised=True)
    check(f"{precision}_ds_ddpm_p_mean", mean, g["mean"], tol)
    assert np.array_equal(var.cpu().numpy(), g["variance"]) and np.array_equal(logvar.cpu().numpy(), g["log_variance"])
    # p_sample draws as noise_like does: one [B, 1, M, T] draw, or one row repeated over the batch; t = 0 adds none of it
    sigma = torch.from_numpy(gd._ddpm_tables[4])[t].reshape(B, 1, 1, 1).cuda()
    for rep in (False, True):
        torch.manual_seed(77)
        y = gd.p_sample(x, t, cond, clip_denoised=True, repeat_noise=rep)
        state = torch.cuda.get_rng_state()
        torch.manual_seed(77)
        z = torch.randn((1 if rep else B, 1, 80, x.shape[3]), device="cuda").expand(B, -1, -1, -1).contiguous()
        assert torch.equal(torch.cuda.get_rng_state(), state)
        assert torch.equal(y, net.ddpm_update(x, eps, t, gd._ddpm_tables, z))
        assert torch.equal(y[0], mean[0]) and not torch.equal(y[1], mean[1])
        if rep:     # rows 1 and 2 carry the same draw, scaled by their own sigma
            r1, r2 = (y[1] - mean[1]) / sigma[1], (y[2] - mean[2]) / sigma[2]
            assert float((r1 - r2).abs().max()) < 1e-4
    from audiogpt_amd._lib import MaaError
    with pytest.raises(MaaError, match="outside"):
        net.ddpm_update(x, eps, torch.tensor([0, 100, 5]), gd._ddpm_tables, z)


def test_refusals_carry_their_reason(rig):
    from audiogpt_amd import _lib as L
    ctx, net = rig("f32", DIL1)
    tabs = tables(DIL1)
    x, cond = torch.zeros(1, 1, 80, 4), torch.zeros(1, 256, 4)
    z = lambda n, B=1, T=4: torch.zeros(n, B, 1, 80, T)    # noqa: E731
    with pytest.raises(L.MaaError, match="at most 256 samples"):
        net.ddpm_sample(torch.zeros(257, 1, 80, 1), torch.zeros(257, 256, 1), tabs, 1, 1, z(1, 257, 1))
    with pytest.raises(L.MaaError, match="outside the schedule"):
        net.ddpm_sample(x, cond, tabs, 100, 2, z(2))
    with pytest.raises(L.MaaError, match="past t = 0"):
        net.ddpm_sample(x, cond, tabs, 2, 4, z(4))
    with pytest.raises(L.MaaError, match="at least 1"):
        net.ddpm_sample(x, cond, tabs, 2, 0, z(0))
    with pytest.raises(L.MaaError, match="cond"):
        net.ddpm_sample(x, torch.zeros(1, 256, 5), tabs, 2, 1, z(1))
    with pytest.raises(L.MaaError, match="noise"):
        net.ddpm_sample(x, cond, tabs, 2, 2, z(1))
    # the library refuses the same on its own (a caller of the C ABI has no Python wrapper in front)
    xd, cd, zd = x.cuda(), cond.cuda(), z(4).cuda()
    ptrs = [np.ascontiguousarray(t).ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for t in tabs]

    def status(B=1, T=4, start=3, n=4, timesteps=100, cond=cd, noise=zd, tab0=ptrs[0]):
        a = L.maa_ds_ddpm_args()
        a.B, a.T, a.start, a.n, a.timesteps, a.clip_denoised, a.use_graph = B, T, start, n, timesteps, 1, 1
        a.d_cond, a.d_noise = (cond.data_ptr() if cond is not None else None), (noise.data_ptr() if noise is not None else None)
        a.h_sqrt_recip_ac, a.h_sqrt_recipm1_ac, a.h_coef1, a.h_coef2, a.h_sigma = [tab0] + ptrs[1:]
        with ctx.lock:
            st = ctx.lib.maa_ds_ddpm_sample(ctx.h, net.h, ctypes.byref(a), L.dptr(xd))
            return st, ctx.lib.maa_last_error().decode()
    for kw, reason in ((dict(B=257), "at most 256 samples"), (dict(start=100), "outside the schedule"), (dict(start=2), "past t = 0"),
                       (dict(n=0), "at least 1"), (dict(cond=None), "d_cond is missing"), (dict(noise=None), "d_noise is missing"),
                       (dict(tab0=None), "tables are missing")):
        st, msg = status(**kw)
        assert st < 0 and reason in msg, (kw, st, msg)
    assert torch.equal(xd, x.cuda())
    st, msg = status()
    assert st == 0, msg
