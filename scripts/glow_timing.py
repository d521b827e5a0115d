"""What the Glow post-net costs per utterance on the device: wall time per PostGlow.infer at T = 1000 frames, B = 1 and B = 8, for
GenerSpeech's configuration (8 blocks, H = 128, 1104 conditioning channels) and PortaSpeech's (12 blocks, H = 192, 272), seeded
random weights, bf16x3, one process and one context.

    python scripts/glow_timing.py [OUT=profiles/glow_timing.txt]

Times are a host clock around one infer() that ends in a synchronise of the context's stream, 20 calls after 3 warm-up calls per
shape; the latent is the caller's, already on the device, so the window holds the conditioning's concatenation (torch) and the
library call, not the host's draw.  The launch counts and the launch-time shares come from one more call of each shape under the
library's per-launch timer (hipEvent pairs, eager), taken after the wall times.  Nothing about this path had been measured
before: the file states the numbers and claims no target."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C
from audiogpt_amd.backend import Context
from audiogpt_amd.generspeech import PostGlow

T, CALLS, WARMUP = 1000, 20, 3


def inputs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    H = cfg["hidden_size"]
    r = lambda *s: torch.randn(*s, generator=g).cuda()          # noqa: E731
    parts = [r(B, T, 80), r(B, T, H)]
    if cfg["n_cond_vectors"]:
        parts += [r(B, 1, H), r(B, 1, H), r(B, T, H)]
    return parts, r(B, 80, T) * cfg["noise_scale"]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/glow_timing.txt"
    ctx = Context("cuda:0", precision="bf16x3")
    text = ["Glow post-net in reverse: wall time per PostGlow.infer, one MI355X, one process, one context", "",
            "command: python scripts/glow_timing.py",
            "shapes:  T = %d frames (%d squeezed rows per sample), bf16x3, seeded random weights, the caller's z on the device" % (T, T // 2),
            "timing:  host clock around infer() + a synchronise of the context's stream; %d calls after %d warm-up calls" % (CALLS, WARMUP),
            "launches: one further call under the library's per-launch timer (its sum of launch durations is device time, not wall time)",
            ""]
    for label, cfg in (("GenerSpeech (C.GENERSPEECH_POST_GLOW)", C.GENERSPEECH_POST_GLOW),
                       ("PortaSpeech (C.PORTASPEECH_POST_GLOW)", C.PORTASPEECH_POST_GLOW)):
        post = PostGlow(cfg, ctx=ctx)
        for B in (1, 8):
            parts, z = inputs(cfg, B, 5)

            def call():
                out = post.infer(*parts, z=z)
                ctx.synchronize()
                return out

            for _ in range(WARMUP):
                out = call()
            assert bool(torch.isfinite(out).all())
            ms = []
            for _ in range(CALLS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            ctx.prof_begin()
            call()
            rows = ctx.prof_end()
            dev = sum(r["ms"] for r in rows.values())
            n = sum(r["launches"] for r in rows.values())
            text.append("%-40s B = %d: median %8.3f ms  min %8.3f  max %8.3f  per call; %d launches, %8.3f ms summed launch time" % (
                label, B, statistics.median(ms), min(ms), max(ms), n, dev))
            for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:6]:
                text.append("    %-44s %5d launches %9.3f ms  %6.2f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / dev))
        post.post_flow.net.close()
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
