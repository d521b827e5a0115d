"""Golden vectors of DiffSinger's ancestral sampling branch, from the REFERENCE's own class (run in the build container only).

    python tests/golden/make_golden_ds_ddpm.py      # needs /root/reference; writes tests/golden/ds_ddpm_*.npz

The real `shallow_diffusion_tts.GaussianDiffusion` / `OfflineGaussianDiffusion` (NeuralSeq/modules/diff/) are constructed on the
CPU with the stub-module approach of make_golden.py::diffsinger_case: `utils.hparams` is a plain dict, `FastSpeech2` a module
that returns a prepared `ret` dict, so the real `forward(infer=True)` runs with `pndm_speedup` unset.  The module is loaded
afresh per case: `linear_beta_schedule` binds hparams['max_beta'] as a default argument at import.  Weights are
`WT.make_diffnet_state_dict(cfg, seed=7)` and are not stored.  Every draw the reference makes is recorded (torch.randn /
torch.randn_like are wrapped while its code runs), in the order it makes them.

Each chain is also run once in float64 on the same draws; the largest fp32 - fp64 difference per step is printed: the
reference's own rounding, the floor under the gates of tests/test_gpu_ds_ddpm.py.
"""
import importlib.util
import inspect
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
NS = os.path.join("/root/reference", "NeuralSeq")

from audiogpt_amd import config as C          # noqa: E402
from audiogpt_amd import weights as WT         # noqa: E402

SPEC_MIN, SPEC_MAX = [-6.0] * 80, [1.5] * 80


class FS2Stub(torch.nn.Module):
    """Stands in for modules.fastspeech.fs2.FastSpeech2: returns the `ret` dict set on it (decoder_inp [B, T, H], mel_out)."""

    def __init__(self, phone_encoder, out_dims):
        super().__init__()
        self.ret = None

    def forward(self, *args, **kwargs):
        return dict(self.ret)


def load_reference(hp):
    """(net module, shallow_diffusion_tts module) of the reference with `hp` as utils.hparams.hparams."""
    stubs = {"utils": {}, "utils.hparams": {"hparams": hp}, "modules": {}, "modules.diff": {}, "modules.fastspeech": {},
             "modules.fastspeech.fs2": {"FastSpeech2": FS2Stub}, "modules.diffsinger_midi": {},
             "modules.diffsinger_midi.fs2": {"FastSpeech2MIDI": FS2Stub}}
    saved = {k: sys.modules.get(k) for k in stubs}
    for k, attrs in stubs.items():
        m = types.ModuleType(k)
        m.__path__ = []
        for a, v in attrs.items():
            setattr(m, a, v)
        sys.modules[k] = m

    def load(modname, rel):
        sp = importlib.util.spec_from_file_location(modname, os.path.join(NS, rel))
        m = importlib.util.module_from_spec(sp)
        sys.modules[modname] = m
        sp.loader.exec_module(m)
        return m
    try:
        load("modules.diff.diffusion", "modules/diff/diffusion.py")
        net = load("modules.diff.net", "modules/diff/net.py")
        sdt = load("modules.diff.shallow_diffusion_tts", "modules/diff/shallow_diffusion_tts.py")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for k in ("modules.diff.diffusion", "modules.diff.net", "modules.diff.shallow_diffusion_tts"):
            sys.modules.pop(k, None)
    return net, sdt


def hparams_of(cfg, **extra):
    hp = dict(hidden_size=cfg["hidden_size"], residual_layers=cfg["residual_layers"], residual_channels=cfg["residual_channels"],
              dilation_cycle_length=cfg["dilation_cycle_length"], keep_bins=80)
    for k in ("schedule_type", "max_beta", "gaussian_start"):
        if cfg.get(k) is not None:
            hp[k] = cfg[k]
    hp.update(extra)
    assert not hp.get("pndm_speedup")
    return hp


def build(cfg, cls="GaussianDiffusion", **extra):
    net, sdt = load_reference(hparams_of(cfg, **extra))
    denoise = net.DiffNet(cfg["in_dims"]).eval()
    denoise.load_state_dict(WT.make_diffnet_state_dict(cfg, seed=7), strict=True)
    gd = getattr(sdt, cls)(None, cfg["in_dims"], denoise, timesteps=cfg["timesteps"], K_step=cfg["K_step"], loss_type="l1",
                           spec_min=SPEC_MIN, spec_max=SPEC_MAX).eval()
    return gd, sdt


class RecordDraws:
    """Records every torch.randn / torch.randn_like made inside the block, in order."""

    def __enter__(self):
        self.draws = []
        self._randn, self._randn_like = torch.randn, torch.randn_like

        def randn(*a, **k):
            z = self._randn(*a, **k)
            self.draws.append(z.detach().clone())
            return z

        def randn_like(*a, **k):
            z = self._randn_like(*a, **k)
            self.draws.append(z.detach().clone())
            return z
        torch.randn, torch.randn_like = randn, randn_like
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like = self._randn, self._randn_like


def chain(gd, sdt, x_T, cond, K, clip, noise=None, dtype=torch.float32):
    """The loop of forward (:270-271) through the reference's p_sample; noise None: drawn (and returned); else replayed."""
    B = x_T.shape[0]
    inter, eps0 = [], []
    hook = gd.denoise_fn.register_forward_hook(lambda m, i, o: eps0.append(o.detach().clone()) if not eps0 else None)
    orig = sdt.noise_like
    it = iter(noise) if noise is not None else None
    if it is not None:
        sdt.noise_like = lambda shape, device, repeat=False: next(it).to(dtype)
    default = torch.get_default_dtype()
    torch.set_default_dtype(dtype)          # (the step embedding builds its frequencies in the default dtype)
    try:
        with RecordDraws() as rec, torch.no_grad():
            x = x_T.to(dtype)
            for i in reversed(range(0, K)):
                x = gd.p_sample(x, torch.full((B,), i, dtype=torch.long), cond.to(dtype), clip_denoised=clip)
                inter.append(x.clone())
    finally:
        torch.set_default_dtype(default)
        sdt.noise_like = orig
        hook.remove()
    return torch.stack(inter), (torch.stack(rec.draws) if noise is None else noise), eps0[0]


def chain_case(tag, cfg, B, T, K, clips=(True,), seed=21):
    """x_T / cond seeded; the chain with every clip setting on ONE set of draws; fp64 rerun for the reference's own rounding."""
    cfg = dict(cfg, K_step=K)
    gd, sdt = build(cfg)
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, cfg["hidden_size"], T, generator=g)
    x_T = torch.randn(B, 1, cfg["in_dims"], T, generator=g)
    out = dict(cond=cond.numpy(), x_T=x_T.numpy(), K_step=K)
    noise = None
    torch.manual_seed(seed + 1)
    gd64 = None
    for clip in clips:
        inter, noise, eps0 = chain(gd, sdt, x_T, cond, K, clip, noise)
        if gd64 is None:
            gd64, sdt64 = build(cfg)
            gd64 = gd64.double()
        inter64, _, _ = chain(gd64, sdt64, x_T, cond, K, clip, noise, torch.float64)
        d = (inter.double() - inter64).abs().flatten(1).max(1).values
        sfx = "" if clip else "_noclip"
        out["x_inter" + sfx] = inter.numpy()
        out["eps0"] = eps0.numpy()
        line = "%s clip=%d  fp32-fp64 per step: %s  max %.2e" % (tag, clip, " ".join("%.1e" % v for v in d.tolist()), float(d.max()))
        if clip:
            # elements the clamp changes: x_recon of each step, recomputed from the recorded trajectory in float64
            n_clamped, xs = 0, torch.cat([x_T[None].double(), inter64[:-1]])
            torch.set_default_dtype(torch.float64)
            with torch.no_grad():
                for j, i in enumerate(reversed(range(K))):
                    t = torch.full((B,), i, dtype=torch.long)
                    xr = gd64.predict_start_from_noise(xs[j], t, gd64.denoise_fn(xs[j], t, cond.double()))
                    n_clamped += int((xr.abs() > 1).sum())
            torch.set_default_dtype(torch.float32)
            line += "  clamped %d of %d" % (n_clamped, K * x_T.numel())
        print(line)
    out["noise"] = noise.numpy()
    return out


def schedule_case():
    out = {}
    for tag, cfg in (("linear100", dict(timesteps=100, schedule_type="linear", max_beta=0.06)),
                     ("cosine100", dict(timesteps=100)),
                     ("linear1000", dict(timesteps=1000, schedule_type="linear", max_beta=0.02))):
        gd, sdt = build({**C.DIFFSINGER_POPCS_BETA6, "schedule_type": None, "max_beta": None, **cfg})
        for k, v in gd.named_buffers():
            if k not in ("spec_min", "spec_max"):
                out[tag + "." + k] = v.numpy()
    names = ("q_mean_variance", "predict_start_from_noise", "q_posterior", "p_mean_variance", "p_sample", "q_sample", "norm_spec",
             "denorm_spec")
    out["signatures"] = np.asarray(json.dumps({n: str(inspect.signature(getattr(sdt.GaussianDiffusion, n))) for n in names}))
    return out


def forward_infer_case(seed=5):
    """forward(infer=True) itself through the fs2 stub; the global generator is seeded, every draw recorded in order."""
    B, T, K = 2, 24, 8
    base = dict(C.DIFFSINGER_POPCS_BETA6, K_step=K)
    g = torch.Generator().manual_seed(seed)
    mel = torch.rand(B, T, 80, generator=g) * 6.0 - 5.0
    dec = torch.randn(B, T, base["hidden_size"], generator=g)
    mel2ph = torch.ones(B, T, dtype=torch.long)
    mel2ph[0, T - 5:] = 0
    mel2ph[1, :2] = 0
    out = dict(fs2_mel=mel.numpy(), decoder_inp=dec.numpy(), mel2ph=mel2ph.numpy(), K_step=K, seed=seed)
    tokens = torch.zeros(B, 4, dtype=torch.long)
    for tag, cls, gs, m2p in (("plain", "GaussianDiffusion", False, None), ("gstart", "GaussianDiffusion", True, None),
                              ("mel2ph", "GaussianDiffusion", False, mel2ph), ("offline", "OfflineGaussianDiffusion", False, mel2ph)):
        gd, sdt = build(dict(base, gaussian_start=gs), cls=cls)
        gd.fs2.ret = dict(decoder_inp=dec, mel_out=mel)
        torch.manual_seed(seed)
        ref_mels = [mel, mel] if cls == "OfflineGaussianDiffusion" else None
        with RecordDraws() as rec, torch.no_grad():
            ret = gd(tokens, mel2ph=m2p, ref_mels=ref_mels, infer=True)
        shapes = [tuple(z.shape) for z in rec.draws]
        want = [(B, 1, 80, T)] * (1 + int(gs) + K)
        assert shapes == want, (shapes, want)
        out[tag + ".mel_out"] = ret["mel_out"].numpy()
        out[tag + ".draws"] = torch.stack(rec.draws).numpy()          # q_sample, [gaussian_start], then one per step
    return out


def p_sample_t_case(seed=9):
    """p_sample with a timestep per sample (0 among them), repeat_noise False and True."""
    B, T = 3, 16
    cfg = dict(C.DIFFSINGER_POPCS_BETA6)
    gd, sdt = build(cfg)
    g = torch.Generator().manual_seed(seed)
    cond = torch.randn(B, cfg["hidden_size"], T, generator=g)
    x = torch.randn(B, 1, 80, T, generator=g)
    t = torch.tensor([0, 37, 99], dtype=torch.long)
    out = dict(cond=cond.numpy(), x=x.numpy(), t=t.numpy())
    for tag, rep in (("each", False), ("repeat", True)):
        torch.manual_seed(seed)
        with RecordDraws() as rec, torch.no_grad():
            y = gd.p_sample(x, t, cond, clip_denoised=True, repeat_noise=rep)
        assert len(rec.draws) == 1 and rec.draws[0].shape[0] == (1 if rep else B)
        out[tag + ".noise"] = rec.draws[0].numpy()
        out[tag + ".out"] = y.numpy()
    with torch.no_grad():
        mean, var, logvar = gd.p_mean_variance(x, t, cond, clip_denoised=True)
    out.update(mean=mean.numpy(), variance=var.numpy(), log_variance=logvar.numpy())
    return out


def main():
    lin = C.DIFFSINGER_DS100_ADJ_REL            # timesteps 100, max_beta 0.06, dilation cycle 4
    cases = {
        "ds_ddpm_schedule": schedule_case(),
        "ds_ddpm_b2_k8": chain_case("b2_k8", lin, 2, 48, 8, clips=(True, False)),
        "ds_ddpm_cosine_k8": chain_case("cosine_k8", dict(lin, schedule_type=None, max_beta=None), 1, 48, 8),
        "ds_ddpm_forward_infer": forward_infer_case(),
        "ds_ddpm_p_sample_t": p_sample_t_case(),
    }
    rag = chain_case("ragged_b3_t33", C.DIFFSINGER_POPCS_BETA6, 3, 33, 6)
    one = chain_case("ragged_t1", C.DIFFSINGER_POPCS_BETA6, 1, 1, 3)
    cases["ds_ddpm_ragged"] = dict({"t33." + k: v for k, v in rag.items()}, **{"t1." + k: v for k, v in one.items()})
    for name, arrays in cases.items():
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(name, "%d bytes" % os.path.getsize(path))
    if "--full" in sys.argv:        # the whole 100-step chain: figures only, nothing stored
        chain_case("full_k100", lin, 1, 48, 100)


if __name__ == "__main__":
    main()
