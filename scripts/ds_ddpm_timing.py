"""What one step of DiffSinger's ancestral chain costs on the device: DiffNet.ddpm_sample over fixed noise, 200 steps of the
1000-step schedule (C.DIFFSINGER_DS1000's denoiser, T = 1000 frames, bf16x3, graph on), at B = 1 and B = 8.

    python scripts/ds_ddpm_timing.py [OUT=profiles/ds_ddpm_timing.txt] [ROUNDS=3] [PARENT=<checkout of the parent commit, built>]
    python scripts/ds_ddpm_timing.py --plms-step      # one line: ms per denoiser evaluation of the PLMS loop at B = 1 and B = 8

The yardstick is the PLMS loop's step at the same shapes (plms_sample with interval 1 over the same 200 timesteps: 200 steps, 201
denoiser evaluations -- the first step takes two): both steps are one DiffNet evaluation, one small kernel and the advance.  With
PARENT the yardstick is the parent commit's: `--plms-step` is run twice from that checkout (cwd decides which package is imported)
and the difference of the two runs is its run-to-run spread; without PARENT the file says that the yardstick was not measured.
Times are host wall time around one call that ends synchronised, two warm-up calls first.  The step kernel's own time comes from
the library's per-kernel timer over an eager 10-step chain."""
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd.backend import Context, DiffNet

T, K, BATCHES = 1000, 200, (1, 8)
CFG = C.DIFFSINGER_DS1000


def _timed(f, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def _inputs(B):
    g = torch.Generator().manual_seed(B)
    return torch.randn(B, 1, CFG["in_dims"], T, generator=g).cuda(), torch.randn(B, CFG["hidden_size"], T, generator=g).cuda()


def _net():
    ctx = Context("cuda:0", precision="bf16x3")
    return ctx, DiffNet(ctx, CFG, WT.make_diffnet_state_dict(CFG, seed=7))


def plms_step(net, B, rounds=3):
    """ms per denoiser evaluation of the PLMS loop (interval 1 over K timesteps), each timed call."""
    import numpy as np
    ac = np.cumprod(1.0 - np.linspace(1e-4, CFG["max_beta"], CFG["timesteps"])).astype(np.float32)
    x, cond = _inputs(B)
    f = lambda: net.plms_sample(x, cond, ac, K, 1)    # noqa: E731
    f()
    f()
    return [1e3 * t / (K + 1) for t in _timed(f, rounds)]


def main():
    args = list(sys.argv[1:])
    if args and args[0] == "--plms-step":
        ctx, net = _net()
        print("plms_ms_per_step " + " ".join("B%d %.4f" % (B, statistics.mean(plms_step(net, B))) for B in BATCHES))
        return
    out_path = args[0] if len(args) > 0 else "profiles/ds_ddpm_timing.txt"
    rounds = int(args[1]) if len(args) > 1 else 3
    parent = args[2] if len(args) > 2 else None
    from audiogpt_amd.diffsinger import schedule_buffers
    b = schedule_buffers(CFG["timesteps"], "linear", CFG["max_beta"])
    tabs = (b["sqrt_recip_alphas_cumprod"], b["sqrt_recipm1_alphas_cumprod"], b["posterior_mean_coef1"], b["posterior_mean_coef2"],
            (0.5 * torch.from_numpy(b["posterior_log_variance_clipped"])).exp().numpy())
    ctx, net = _net()
    mine, own = {}, {}
    for B in BATCHES:
        x, cond = _inputs(B)
        noise = torch.randn(K, B, 1, CFG["in_dims"], T, device="cuda")
        f = lambda: net.ddpm_sample(x, cond, tabs, K - 1, K, noise)    # noqa: E731
        f()
        f()
        mine[B] = [1e3 * t / K for t in _timed(f, rounds)]
        own[B] = plms_step(net, B, rounds)
        del noise
    text = ["DiffSinger ancestral sampling: time per step of the device loop, one MI355X, one process", "",
            "command: python scripts/ds_ddpm_timing.py  (%d timed calls after 2 warm-up calls each)" % rounds,
            "shapes:  x [B, 1, 80, %d], cond [B, 256, %d], DIFFSINGER_DS1000's denoiser, bf16x3, hipGraph on; ancestral: %d steps over"
            % (T, T, K),
            "         fixed noise (t = %d .. 0 of 1000); PLMS: interval 1 over the same timesteps, %d steps = %d evaluations" % (K - 1, K, K + 1),
            "", "ms per step (ancestral) / per denoiser evaluation (PLMS), mean and each call:"]
    for B in BATCHES:
        text += ["  B = %d  ancestral          %8.4f   (calls: %s)" % (B, statistics.mean(mine[B]), " ".join("%.4f" % t for t in mine[B])),
                 "  B = %d  this build's PLMS  %8.4f   (calls: %s)" % (B, statistics.mean(own[B]), " ".join("%.4f" % t for t in own[B]))]
    slower = []
    if not parent:
        text.append("  parent commit's PLMS yardstick: NOT MEASURED (no PARENT checkout given): the ancestral steps above are unjudged")
    else:
        got = []
        for _ in range(2):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plms-step"], cwd=parent, capture_output=True, text=True,
                               timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("plms_ms_per_step")]
            if r.returncode != 0 or not line:
                text.append("  parent commit's PLMS yardstick: NOT MEASURED (%s): the ancestral steps above are unjudged"
                            % (r.stderr.strip().splitlines() or ["no output"])[-1][:160])
                break
            w = line[0].split()
            got.append({int(w[i][1:]): float(w[i + 1]) for i in range(1, len(w), 2)})
        if len(got) == 2:
            for B in BATCHES:
                p = [got[0][B], got[1][B]]
                spread = abs(p[0] - p[1])
                d = statistics.mean(mine[B]) - statistics.mean(p)
                if d > 2 * spread:
                    slower.append("B = %d" % B)
                text.append("  B = %d  parent commit's PLMS %8.4f %8.4f  (two runs; spread %.4f)   ancestral - parent = %+.4f ms: %s"
                            % (B, p[0], p[1], spread, d,
                               "within twice the spread" if d <= 2 * spread else "SLOWER than the parent's step by more than twice the spread"))
    # the step kernel's own time: eager 10-step chain under the per-kernel timer
    for B in BATCHES:
        x, cond = _inputs(B)
        noise = torch.randn(10, B, 1, CFG["in_dims"], T, device="cuda")
        net.ddpm_sample(x, cond, tabs, 9, 10, noise, use_graph=False)
        ctx.prof_begin()
        net.ddpm_sample(x, cond, tabs, 9, 10, noise, use_graph=False)
        rows = ctx.prof_end()
        total = sum(r["ms"] for r in rows.values())
        text += ["", "B = %d: eager 10-step chain under the per-kernel timer (sum of launch durations %.3f ms)%s:"
                 % (B, total, "; the ancestral step is slower than the parent's PLMS step by more than twice the spread at %s -- this "
                    "table shows where a step's time goes" % " and ".join(slower) if slower else "")]
        for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:10]:
            text.append("  %-44s %5d launches %9.3f ms  %6.3f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
        for k in rows:
            if k.startswith("ds_ddpm_step_kernel"):
                text.append("  -> %-41s %5d launches %9.3f ms  %6.3f %% of the launches' time, %.2f us per launch"
                            % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total,
                               1e3 * rows[k]["ms"] / max(rows[k]["launches"], 1)))
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
