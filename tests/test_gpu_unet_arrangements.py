"""The UNet executor's arrangements of a guided step on transformer UNets the other model tests never build.

Every UNet config elsewhere in the suite has transformer_depth = 1 and attention at ds = 1, so three branches of csrc/unet.cpp
never ran under test: the transformer blocks after a SpatialTransformer's first, the one-stream shared prefix with several
input blocks in front of the first transformer (every skip tensor written twice), and two lanes on a transformer UNet whose
first transformer is not input block 1 (prefix_ok() false: both lanes run the whole network).  The configs here are small
T2A variants (64 channels, head widths 32 and 64, both covered by the flash kernel):
  depth2           transformer_depth = 2, attention at ds = 1 and 2
  attn_ds2         attention at ds = 2 only
  depth2_attn_ds2  both
Inputs: x [2, 4, 8, 16], t = [10, 500], context [2, 5, 64]; weights make_unet_state_dict(cfg, seed=7).  The references are the
CPU oracle in float32 (oracle.unet.unet_forward; oracle.ddim.ddim_sample driving it), computed once per config.

Gates: one forward rel-max 1e-4 (test_gpu_models.test_unet_t2a_matches_reference's), the 3-step guided DDIM latent rel-max 1e-3
(the project's DDIM-latent gate, tests/test_gpu_models.py).

MAA_CFG_SHARED is read from the environment by reload_tuning() alone, which drops every kept step graph, so "a kept graph is not
replayed across a change of the knob" cannot be staged from here; the loop's graph key carries the share mode and the lane count
all the same (csrc/ddim.cpp Loop::key)."""
import functools
import os

import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests.util import check

pytestmark = pytest.mark.gpu

BASE = dict(C.UNET_T2A, model_channels=64, num_heads=2, context_dim=64)
CONFIGS = {"depth2": dict(BASE, transformer_depth=2),
           "attn_ds2": dict(BASE, attention_resolutions=(2,)),
           "depth2_attn_ds2": dict(BASE, transformer_depth=2, attention_resolutions=(2,))}
SCALE = 1.5
# a 999-step training schedule: uniform spacing (T // S) then gives exactly three DDIM steps, 1 / 334 / 667
T_TRAIN, S = 999, 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """Weights, inputs and the oracle's answers for one config (shared by every test of it, never modified)."""
    from oracle import ddim as O_ddim
    from oracle import unet as O_unet
    cfg = CONFIGS[name]
    sd = WT.make_unet_state_dict(cfg, seed=7)
    g = torch.Generator().manual_seed(71)
    x = torch.randn(2, 4, 8, 16, generator=g)
    t = torch.tensor([10.0, 500.0])
    ctx = torch.randn(2, 5, 64, generator=g)
    uncond = torch.randn(2, 5, 64, generator=g)
    ac = O_ddim.alphas_cumprod(T_TRAIN, C.LDM_T2A["linear_start"], C.LDM_T2A["linear_end"])
    steps = O_ddim.ddim_timesteps(S, T_TRAIN)
    assert len(steps) == S
    a, ap, _, _ = O_ddim.ddim_tables(ac, steps)
    with torch.no_grad():
        eps = O_unet.unet_forward(sd, cfg, x, t, ctx)
        z = O_ddim.ddim_sample(lambda xx, tt, cc: O_unet.unet_forward(sd, cfg, xx, tt, cc), ac, S, x, ctx, uncond, SCALE)
    for ref in (eps, z):
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    return dict(cfg=cfg, sd=sd, x=x, t=t, ctx=ctx, uncond=uncond, steps=steps, a=a.numpy(), ap=ap.numpy(), eps=eps, z=z)


class _Model:
    """A context and the config's UNet; the environment knob and the lane setting are put back on exit."""

    def __init__(self, name, precision):
        self.name, self.precision = name, precision

    def __enter__(self):
        from audiogpt_amd.backend import Context, UNet
        k = _case(self.name)
        self.c = Context("cuda:0", precision=self.precision)
        self.u = UNet(self.c, k["cfg"], k["sd"])
        return self.c, self.u, k

    def __exit__(self, *exc):
        from audiogpt_amd.backend import reload_tuning
        os.environ.pop("MAA_CFG_SHARED", None)
        reload_tuning()
        self.c.set_cfg_split(None)
        self.u.close()
        self.c.close()


def _arrange(c, shared, lanes):
    from audiogpt_amd.backend import reload_tuning
    os.environ["MAA_CFG_SHARED"] = shared
    reload_tuning()
    c.set_cfg_split(lanes)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_one_forward_matches_the_oracle(name, precision):
    """The blocks after a SpatialTransformer's first (their own norms, projections and K/V slot) against the oracle."""
    with _Model(name, precision) as (c, u, k):
        y = u(k["x"], k["t"], k["ctx"])
        r = check("unet_arr_%s_%s_forward" % (name, precision), y, k["eps"], 1e-4)
        print("forward %s %s: rel-max %.3e, max |eps| %.3f" % (name, precision, r, float(k["eps"].abs().max())))


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_guided_ddim_is_the_same_under_every_arrangement(name, precision):
    """A guided 3-step DDIM (scale 1.5, B = 2, uncond != cond) under MAA_CFG_SHARED in {0, 1} x one stream / two lanes x eager /
    graph / the kept graph again: every latent within the DDIM gate of the oracle, and all twelve equal bit for bit (every kernel
    is batch-invariant at these shapes on the parent of the commit that added this file as well: no K split differs between the
    half and the full batch)."""
    out = {}
    with _Model(name, precision) as (c, u, k):
        kw = dict(cond=k["ctx"], uncond=k["uncond"], scale=SCALE)
        for shared in ("0", "1"):
            for lanes in (False, True):
                _arrange(c, shared, lanes)
                for how, graph in (("eager", False), ("graph", True), ("again", True)):
                    out[shared, lanes, how] = u.ddim_sample(k["x"], k["steps"], k["a"], k["ap"], use_graph=graph, **kw).cpu()
    ref = out["0", False, "eager"]
    differ = [key for key, v in out.items() if not torch.equal(v, ref)]
    for key, v in out.items():
        r = check("unet_arr_%s_%s_ddim_%s_%d_%s" % ((name, precision) + key), v, k["z"], 1e-3)
        print("ddim %s %s %s: rel-max %.3e" % (name, precision, key, r))
    assert not differ, ("arrangements differ from MAA_CFG_SHARED=0 on one stream, eager", differ)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_prefix_is_shared_where_it_should_be(name, precision):
    """One eager guided step under the profiler.  Attention at ds = 1: fewer FLOPs with the shared prefix, on one stream and as
    two lanes.  Attention at ds = 2 only: fewer on one stream (conv_in, two ResBlocks, the downsample, a third ResBlock and the
    transformer's first half on one half of the batch); the same as two lanes, where the hand-over is written for the transformer
    in input block 1 alone (prefix_ok() false) and both lanes run the whole network."""
    flops = {}
    with _Model(name, precision) as (c, u, k):
        kw = dict(cond=k["ctx"], uncond=k["uncond"], scale=SCALE)
        for shared in ("0", "1"):
            for lanes in (False, True):
                _arrange(c, shared, lanes)
                u.ddim_sample(k["x"], k["steps"][:1], k["a"][:1], k["ap"][:1], use_graph=False, **kw)      # (sizes the workspace)
                c.prof_begin()
                u.ddim_sample(k["x"], k["steps"][:1], k["a"][:1], k["ap"][:1], use_graph=False, **kw)
                flops[shared, lanes] = sum(v["flops"] for v in c.prof_end().values())
    print("flops %s %s: %s" % (name, precision, flops))
    assert min(flops.values()) > 0, flops
    assert flops["1", False] < flops["0", False], flops
    if 1 in k["cfg"]["attention_resolutions"]:
        assert flops["1", True] < flops["0", True], flops
    else:
        assert flops["1", True] == flops["0", True], flops
