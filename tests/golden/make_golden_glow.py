"""Golden vectors of the Glow post-net run in reverse, from the REFERENCE's own class
`modules.GenerSpeech.model.glow_modules.Glow` (run in the build container only, on the CPU).

    python tests/golden/make_golden_glow.py [name ...]     # writes tests/golden/glow_*.npz and postglow_*.npz (or the named ones)

The class imports through the stubs make_golden_fs2.load_reference installs.  Weights are `WT.make_glow_state_dict(cfg, seed,
coupling_gain)` loaded with strict=True and are never stored: the files keep the configuration, the seed and the gain, and the
state dict's key list with its shapes.  PortaSpeech's copy of the class (modules/commons/normalizing_flow) does not import; it is
the same mathematics and is covered by running this class at ps_flow.yaml's sizes.

Every case is run in fp32 and once more in float64 (the same module, .double()); the largest fp32 - fp64 differences of x, logdet
and every entry of hs are stored as floor_x, floor_logdet and floor_hs [3 n_blocks]: the reference's own rounding, the floor under
the gates of tests/test_glow_host.py.  Asserted here, on the reference alone: floor_x < 1e-5 max|x| (a tenth of the device gate)
and max|x| < 100 -- the couplings' amplification compounds over the blocks, so a case whose draw exceeds that halves its
coupling_gain until it does not.

postglow_gs_t40 is `GenerSpeech.run_post_glow`'s inference branch, called unbound on an object that has only post_flow and
prior_dist, on a stub `ret`; the host's global generator is seeded with `draw_seed` first, so the prior draw is covered."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden_fs2 as G                        # noqa: E402
from audiogpt_amd import config as C               # noqa: E402
from audiogpt_amd import weights as WT              # noqa: E402

GS = C.GENERSPEECH_POST_GLOW
NARROW = dict(GS, in_channels=20, hidden_channels=32, n_blocks=2, n_layers=2, gin_channels=16, share_wn_layers=0)
TINY = dict(NARROW, gin_channels=8)
VARIANTS = dict(GS, hidden_channels=64, kernel_size=5, dilation_rate=2, n_blocks=3, gin_channels=24, share_cond_layers=True,
                share_wn_layers=2, sigmoid_scale=True)
UNCOND = dict(NARROW, hidden_channels=64, n_layers=3, gin_channels=0)
GLOW_KEYS = ("in_channels", "hidden_channels", "kernel_size", "dilation_rate", "n_blocks", "n_layers", "n_split", "n_sqz",
             "gin_channels", "share_cond_layers", "share_wn_layers", "sigmoid_scale")

# name: (cfg, weight seed, B, T, live lengths or None, input seed)
CASES = {
    "glow_gs_t40": (GS, 23, 1, 40, None, 101),
    "glow_gs_b2_t37": (GS, 23, 2, 37, (37, 21), 102),
    "glow_narrow_b2_t300": (NARROW, 24, 2, 300, (300, 155), 103),
    "glow_t2": (TINY, 25, 1, 2, None, 104),
    "glow_t3": (TINY, 25, 1, 3, None, 105),
    "glow_variants_b2_t24": (VARIANTS, 26, 2, 24, (24, 17), 106),
    "glow_uncond_t16": (UNCOND, 27, 1, 16, None, 107),
    "glow_ps_t40": (C.PORTASPEECH_POST_GLOW, 28, 1, 40, None, 108),
}
POSTGLOW = {"postglow_gs_t40": (GS, 23, 1, 40, 109, 1234)}      # cfg, weight seed, B, T, input seed, draw seed


def build(gm, cfg, seed, gain):
    model = gm.Glow(cfg["in_channels"], cfg["hidden_channels"], cfg["kernel_size"], cfg["dilation_rate"], cfg["n_blocks"],
                    cfg["n_layers"], p_dropout=cfg["p_dropout"], n_split=cfg["n_split"], n_sqz=cfg["n_sqz"],
                    sigmoid_scale=cfg["sigmoid_scale"], gin_channels=cfg["gin_channels"], inv_conv_type=cfg["inv_conv_type"],
                    share_cond_layers=cfg["share_cond_layers"], share_wn_layers=cfg["share_wn_layers"]).eval()
    sd = WT.make_glow_state_dict(cfg, seed=seed, coupling_gain=gain)
    model.load_state_dict(sd, strict=True)
    return model, sd


def inputs(cfg, B, T, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, cfg["in_channels"], T, generator=g) * 0.8
    cond = torch.randn(B, cfg["gin_channels"], T, generator=g) if cfg["gin_channels"] else None
    mask = torch.ones(B, 1, T)
    for b, n in enumerate(lengths or ()):
        mask[b, :, n:] = 0.0
    return z, cond, mask


def run(model, z, cond, mask, double=False):
    m = model.double() if double else model
    cast = (lambda t: None if t is None else t.double()) if double else (lambda t: t)
    with torch.no_grad():
        x, logdet, hs = m(cast(z), cast(mask), g=cast(cond), reverse=True, return_hiddens=True)
    return x, logdet, hs


def floors(a, b):
    return float((a[0].double() - b[0]).abs().max()), float((a[1].double() - b[1]).abs().max()), \
        np.array([float((p.double() - q).abs().max()) for p, q in zip(a[2], b[2])])


def settle(gm, cfg, seed, z, cond, mask):
    """The case's model at the largest coupling_gain 1, 1/2, 1/4, .. whose output stays below 100."""
    gain = 1.0
    while True:
        model, sd = build(gm, cfg, seed, gain)
        out = run(model, z, cond, mask)
        if float(out[0].abs().max()) < 100.0:
            return model, sd, out, gain
        gain /= 2.0
        assert gain > 1e-3


def meta(cfg, sd, seed, gain):
    keys = sorted(sd)
    return dict(cfg=np.array([int(cfg[k]) for k in GLOW_KEYS], np.int64), weight_seed=seed, coupling_gain=gain, keys=np.array(keys),
                key_shapes=np.array([",".join(str(s) for s in sd[k].shape) for k in keys]))


def make_case(gm, name):
    cfg, seed, B, T, lengths, in_seed = CASES[name]
    z, cond, mask = inputs(cfg, B, T, lengths, in_seed)
    model, sd, out, gain = settle(gm, cfg, seed, z, cond, mask)
    fx, fl, fh = floors(out, run(build(gm, cfg, seed, gain)[0], z, cond, mask, double=True))
    xmax = float(out[0].abs().max())
    assert fx < 1e-5 * xmax, (name, fx, xmax)
    assert out[0].shape == (B, cfg["in_channels"], 2 * (T // 2)) and len(out[2]) == 3 * cfg["n_blocks"]
    arrays = dict(z=z.numpy(), mask=mask.numpy(), x=out[0].numpy(), logdet=out[1].numpy(), hs=torch.stack(out[2]).numpy(),
                  floor_x=fx, floor_logdet=fl, floor_hs=fh, **meta(cfg, sd, seed, gain))
    if cond is not None:
        arrays["g"] = cond.numpy()
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%s: keys %d gain %g max|x| %.3g floor_x %.2e (%.1e of max) logdet %s floor %.1e  %d bytes" % (
        name, len(sd), gain, xmax, fx, fx / xmax, out[1].numpy(), fl, os.path.getsize(path)))


def make_postglow(gm, hparams, name):
    import modules.GenerSpeech.model.generspeech as gsm
    cfg, seed, B, T, in_seed, draw_seed = POSTGLOW[name]
    coupling_gain = float(np.load(os.path.join(HERE, "glow_gs_t40.npz"))["coupling_gain"])      # case 1's model
    H = cfg["hidden_size"]
    g = torch.Generator().manual_seed(in_seed)
    ret = dict(mel_out=torch.randn(B, T, 80, generator=g), decoder_inp=torch.randn(B, T, H, generator=g),
               spk_embed=torch.randn(B, 1, H, generator=g), emo_embed=torch.randn(B, 1, H, generator=g),
               ref_prosody=torch.randn(B, T, H, generator=g))
    hparams.update(use_txt_cond=cfg["use_txt_cond"], noise_scale=cfg["noise_scale"])
    outs = []
    for double in (False, True):
        model, sd = build(gm, cfg, seed, coupling_gain)
        stub = types.SimpleNamespace(post_flow=model.double() if double else model, prior_dist=torch.distributions.Normal(0, 1))
        r = {k: (v.double() if double else v.clone()) for k, v in ret.items()}
        torch.manual_seed(draw_seed)
        with torch.no_grad():
            if double:      # (the branch draws in fp32 and hands the draw to the flow: cast it where the flow receives it)
                flow = stub.post_flow
                stub.post_flow = lambda zz, m, gg, reverse: flow(zz.double(), m, gg, reverse=reverse)
            gsm.GenerSpeech.run_post_glow(stub, None, True, False, r)
        outs.append(r["mel_out"])
    state_after = torch.get_rng_state()
    torch.manual_seed(draw_seed)
    z = torch.distributions.Normal(0, 1).sample((B, 80, T)) * cfg["noise_scale"]
    assert torch.equal(torch.get_rng_state(), state_after)
    fx = float((outs[0].double() - outs[1]).abs().max())
    xmax = float(outs[0].abs().max())
    assert fx < 1e-5 * xmax and xmax < 100.0, (fx, xmax)
    arrays = dict(mel_out=ret["mel_out"].numpy(), decoder_inp=ret["decoder_inp"].numpy(), spk_embed=ret["spk_embed"].numpy(),
                  emo_embed=ret["emo_embed"].numpy(), ref_prosody=ret["ref_prosody"].numpy(), draw_seed=draw_seed, z=z.numpy(),
                  x=outs[0].numpy(), floor_x=fx, **meta(cfg, sd, seed, coupling_gain))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%s: max|x| %.3g floor_x %.2e  %d bytes" % (name, xmax, fx, os.path.getsize(path)))


def main(names):
    G.load_reference()
    from utils.hparams import hparams
    import modules.GenerSpeech.model.glow_modules as gm
    for name in names or list(CASES) + list(POSTGLOW):
        if name in CASES:
            make_case(gm, name)
        else:
            make_postglow(gm, hparams, name)


if __name__ == "__main__":
    main(sys.argv[1:])
