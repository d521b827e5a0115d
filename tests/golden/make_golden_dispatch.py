"""What the contraction dispatch decides, recorded from the library itself (needs an MI355X).

    python tests/golden/make_golden_dispatch.py     # writes tests/golden/igemm_dispatch.json

For every (model, context) case below: the profile rows of one eager forward with `prof_begin(detail=True)` as
{row name: launches} -- the detail names carry the engine, the tile, the K slices and the problem shape -- and
`workspace_bytes()` after the run (the split-K slabs are borrowed from the workspace, so its size pins the slab sizes).
Weights are the seeded synthetic ones; only names and counts are stored, never values or times.

igemm_dispatch.json was recorded at the commit BEFORE launch_igemm moved into csrc/igemm_dispatch.cpp and pins that move:
tests/test_gpu_dispatch.py replays the cases against it.  Record it again only for a deliberate policy change.

    models     unet_t2a_b2 (the unet_t2a golden's batch), unet_t2a_b16 (the benchmark's guided batch: the tile choice depends
               on M), unet_inpaint (10x106, one sample), vae_decode (latent [1, 4, 10, 78]), hifigan / bigvgan (48 frames)
    contexts   bf16x3, bf16x3 after set_concurrency(3) ("bf16x3_c3"), bf16, f32
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "igemm_dispatch.json")
ROW_CAP = 512          # prof_end returns at most this many rows: a case that reaches it would be truncated
CONTEXTS = [("bf16x3", "bf16x3", None), ("bf16x3_c3", "bf16x3", 3), ("bf16", "bf16", None), ("f32", "f32", None)]


def _models():
    """name -> (make(ctx) -> model, run(model)); the state dicts are built once and shared by the four contexts."""
    from audiogpt_amd import config as C
    from audiogpt_amd import weights as WT
    from audiogpt_amd.backend import UNet, VAE, Vocoder
    g = torch.Generator().manual_seed(0)
    usd = WT.make_unet_state_dict(C.UNET_T2A, seed=0)
    isd = WT.make_unet_state_dict(C.UNET_INPAINT, seed=0)
    vsd = WT.make_vae_state_dict(C.VAE_DDCONFIG, seed=0, with_encoder=False)
    hsd = WT.make_vocoder_state_dict(C.HIFIGAN_16K, seed=0)
    bsd = WT.make_vocoder_state_dict(C.BIGVGAN_16K, seed=0)
    x16, c16 = torch.randn(16, 4, 10, 78, generator=g), torch.randn(16, 77, 1024, generator=g)
    t16 = torch.arange(16, dtype=torch.float32) * 60 + 1
    xi = torch.randn(1, 9, 10, 106, generator=g)
    z = torch.randn(1, 4, 10, 78, generator=g)
    mel = torch.rand(1, 80, 48, generator=g)
    return {
        "unet_t2a_b2": (lambda ctx: UNet(ctx, C.UNET_T2A, usd), lambda m: m(x16[:2], t16[:2], c16[:2])),
        "unet_t2a_b16": (lambda ctx: UNet(ctx, C.UNET_T2A, usd), lambda m: m(x16, t16, c16)),
        "unet_inpaint": (lambda ctx: UNet(ctx, C.UNET_INPAINT, isd), lambda m: m(xi, t16[:1], None)),
        "vae_decode": (lambda ctx: VAE(ctx, C.VAE_DDCONFIG, vsd), lambda m: m.decode(z, 1.0)),
        "hifigan": (lambda ctx: Vocoder(ctx, C.HIFIGAN_16K, hsd), lambda m: m(mel)),
        "bigvgan": (lambda ctx: Vocoder(ctx, C.BIGVGAN_16K, bsd), lambda m: m(mel)),
    }


def record_all():
    """{"<model>/<context>": {"rows": {name: launches}, "workspace_bytes": n}}; a fresh context per case, so that no case's
    workspace depends on the ones before it."""
    from audiogpt_amd.backend import Context
    out = {}
    for mname, (make, run) in _models().items():
        for cname, precision, conc in CONTEXTS:
            ctx = Context("cuda:0", precision=precision)
            if conc is not None:
                ctx.set_concurrency(conc)
            model = make(ctx)
            ctx.prof_begin(detail=True)
            run(model)
            rows = ctx.prof_end()
            assert len(rows) < ROW_CAP, "%s/%s: %d profile rows reach the cap; split this model's run" % (mname, cname, len(rows))
            out["%s/%s" % (mname, cname)] = {"rows": {k: v["launches"] for k, v in sorted(rows.items())},
                                            "workspace_bytes": ctx.workspace_bytes()}
            model.close()
            ctx.close()
    return out


if __name__ == "__main__":
    import time
    t0 = time.time()
    rec = record_all()
    dst = sys.argv[1] if len(sys.argv) > 1 else PATH
    with open(dst, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases, %d rows in all, %.1f s" % (dst, len(rec), sum(len(v["rows"]) for v in rec.values()), time.time() - t0))
