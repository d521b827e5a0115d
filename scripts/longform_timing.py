"""What `split_input_params` costs: MakeAnAudio.generate at 8 prompts x 100 guided DDIM steps (77 tokens, CFG 1.5, bf16x3, graph
on, one batch owning the GPU), three ways in one process:

    a  the native latent 10 x 78
    b  a 10 x 234 latent with the split ks (10, 78), stride (10, 39): 5 crops per sample, 80 UNet rows per guided step
    c  the same 10 x 234 latent evaluated whole (no split), if the UNet accepts it

    python scripts/longform_timing.py [OUT=profiles/longform_timing.txt] [ROUNDS=3]      # on an MI355X, from the repository root

One MakeAnAudio per run so that each keeps its own step graph; two warm-up calls each, then the runs alternate ROUNDS times (host
wall time around one generate call, the device synchronised before and after).  The share of the unfold and fold launches in a
step comes from the library's per-kernel timer over an eager 10-step trajectory of run b."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C
from audiogpt_amd.pipeline import MakeAnAudio

OUT = sys.argv[1] if len(sys.argv) > 1 else "profiles/longform_timing.txt"
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
B, S, SCALE = 8, 100, 1.5
SPLIT = dict(ks=(10, 78), stride=(10, 39), clip_min_weight=0.01, clip_max_weight=0.5, tie_braker=False,
             clip_min_tie_weight=0.01, clip_max_tie_weight=0.5, patch_distributed_vq=False, vqf=8)
g = torch.Generator().manual_seed(0)
c = torch.nn.functional.layer_norm(torch.randn(B, 77, 1024, generator=g), (1024,)).cuda()
uc = torch.nn.functional.layer_norm(torch.randn(B, 77, 1024, generator=g), (1024,)).cuda()
runs, lines = {}, []
for name, W, split in (("a_native_10x78", 78, None), ("b_split_10x234", 234, SPLIT), ("c_whole_10x234", 234, None)):
    m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, precision="bf16x3")
    m.ctx.set_concurrency(1)
    x = torch.randn(B, 4, 10, W, generator=g).cuda()
    f = lambda m=m, x=x, split=split: m.generate(x, c, uc, SCALE, S, split=split)
    try:
        f()
        f()
    except Exception as e:          # (run c only: a UNet that does not take the wide latent is a finding, not a failure)
        if name[0] != "c":
            raise
        lines.append("%-16s not run: %s" % (name, str(e).splitlines()[0][:160]))
        m.close()
        continue
    runs[name] = (m, f, m.audio_seconds(B, 8 * W))
times = {k: [] for k in runs}
torch.cuda.synchronize()
for r in range(ROUNDS):
    for k, (m, f, _) in runs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        times[k].append(time.perf_counter() - t0)
head = ["split_input_params: generate at 8 prompts x 100 guided DDIM steps, one MI355X, all runs in one process",
        "", "command: python scripts/longform_timing.py  (%d timed rounds after 2 warm-up calls each, runs alternated)" % ROUNDS,
        "shapes:  77-token conditioning, CFG 1.5 (two lanes), bf16x3, hipGraph on, set_concurrency(1); VAE decode and HiFi-GAN",
        "         on the whole width; split = ks (10, 78), stride (10, 39): 5 crops per sample, 80 UNet rows per guided step", "",
        "%-16s %10s %10s %10s %16s" % ("run", "audio s", "mean s", "sd s", "audio-seconds/s")]
for k, (m, f, audio) in runs.items():
    v = times[k]
    head.append("%-16s %10.1f %10.4f %10.4f %16.1f" % (k, audio, statistics.mean(v), statistics.stdev(v) if len(v) > 1 else 0.0,
                                                       audio / statistics.mean(v)))
head += lines
# per-step share of the split's own launches: eager 10-step trajectory of run b under the per-kernel timer
m, _, _ = runs["b_split_10x234"]
x = torch.randn(B, 4, 10, 234, generator=g).cuda()
m.sample_latents(x, c, uc, SCALE, 10, use_graph=False, split=SPLIT)
m.ctx.prof_begin()
m.sample_latents(x, c, uc, SCALE, 10, use_graph=False, split=SPLIT)
rows = m.ctx.prof_end()
total = sum(r["ms"] for r in rows.values())
head += ["", "eager 10-step trajectory of run b under the per-kernel timer (sum of launch durations %.2f ms):" % total]
for k in ("split_unfold_kernel", "split_fold_kernel", "split_norm_kernel", "repeat_rows_kernel"):
    if k in rows:
        head.append("  %-22s %4d launches %8.3f ms  %6.3f %% of the launches' time" % (k, rows[k]["launches"], rows[k]["ms"],
                                                                                   100.0 * rows[k]["ms"] / total))
text = "\n".join(head) + "\n"
print(text)
with open(OUT, "w") as fh:
    fh.write(text)
for m, _, _ in runs.values():
    m.close()
