"""PLMS S=25 vs DDIM S=25 vs DDIM S=100 at configs[1] shapes (8 prompts, 77 tokens, CFG 1.5, bf16x3, graph on, one batch
owning the GPU), alternated; one context per trajectory so that each keeps its own step graph.

    python scripts/plms_timing.py [ROUNDS=6]      # on an MI355X, from the repository root; prints one JSON object

Each trajectory is warmed up twice (workspaces sized, step graphs captured), then the three are timed in turn ROUNDS times
(host wall time around one UNet.plms_sample / ddim_sample call, the device synchronised before and after)."""
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C, weights as WT
from audiogpt_amd.backend import Context, UNet
from audiogpt_amd.pipeline import alphas_cumprod_f32, ddim_schedule

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
ldm = C.LDM_T2A
ac = alphas_cumprod_f32(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
g = torch.Generator().manual_seed(0)
x = torch.randn(8, 4, 10, 78, generator=g).cuda()
c = torch.nn.functional.layer_norm(torch.randn(8, 77, 1024, generator=g), (1024,)).cuda()
uc = torch.nn.functional.layer_norm(torch.randn(8, 77, 1024, generator=g), (1024,)).cuda()
sd = WT.make_unet_state_dict(C.UNET_T2A, seed=0)
runs = {}
for name, kind, S in (("plms_s25", "plms", 25), ("ddim_s25", "ddim", 25), ("ddim_s100", "ddim", 100)):
    ctx = Context("cuda:0", precision="bf16x3")
    ctx.set_concurrency(1)
    u = UNet(ctx, C.UNET_T2A, sd)
    steps, a, ap = ddim_schedule(S, ac)
    fn = u.plms_sample if kind == "plms" else u.ddim_sample
    runs[name] = (ctx, u, lambda fn=fn, steps=steps, a=a, ap=ap: fn(x, steps, a, ap, cond=c, uncond=uc, scale=1.5, use_graph=True))
times = {k: [] for k in runs}
for k, (ctx, u, f) in runs.items():       # warm-up: sizes workspaces, captures graphs
    f()
    f()
torch.cuda.synchronize()
for r in range(ROUNDS):
    for k, (ctx, u, f) in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) * 1e3)
res = {k: dict(mean_ms=statistics.mean(v), sd_ms=statistics.stdev(v), n=len(v), all_ms=[round(t, 2) for t in v]) for k, v in times.items()}
p, d = res["plms_s25"]["mean_ms"], res["ddim_s25"]["mean_ms"]
res["plms_s25_over_ddim_s25"] = p / d
res["bound_(S+1)/S*1.03"] = 26 / 25 * 1.03
res["plms_s25_over_ddim_s100"] = p / res["ddim_s100"]["mean_ms"]
print(json.dumps(res, indent=1))
