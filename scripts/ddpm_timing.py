"""What the model's own ancestral (DDPM) sampler costs: MakeAnAudio.generate(sampler="ddpm") at 8 T2A prompts over all 1000
timesteps (77 tokens, bf16x3, graph on, one batch owning the GPU), in one process:

    a  ancestral, unguided, 1000 steps
    b  ancestral, guided at 1.5 (the guidance extension), 1000 steps
    c  for scale: the 100-step guided DDIM run (longform_timing's row a)

    python scripts/ddpm_timing.py [OUT=profiles/ddpm_timing.txt] [ROUNDS=3] [PARENT=<checkout of the parent commit, built>] [BENCH_STEPS=6]
    python scripts/ddpm_timing.py --ddim-steps      # one line: ms per step of the unguided and the guided 100-step DDIM loop

One MakeAnAudio per run so that each keeps its own step graph; two warm-up calls each, then the runs alternate ROUNDS times (host
wall time around one call, the device synchronised before and after).  The per-step times of a and b come from the device loop
alone (UNet.ddpm_sample over fixed noise); their yardstick is the per-step time of the unguided and the guided DDIM loop at the
same batch -- an ancestral step is the same UNet evaluation plus one elementwise kernel.  With PARENT the yardstick is the parent
commit's: `--ddim-steps` is run twice from that checkout (cwd decides which package is imported) and the difference of the two
runs is the job's run-to-run spread; without PARENT the file says that the yardstick was not measured.  Last, the DDIM regression
check: bench.py for this build and for the parent, twice each, alternated (bench_ab).  The share of the step kernel comes from the library's per-kernel timer over an eager
10-step chain."""
import os
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C
from audiogpt_amd.pipeline import MakeAnAudio

B, S, SCALE, T = 8, 100, 1.5, 1000


def _cond():
    g = torch.Generator().manual_seed(0)
    c = torch.nn.functional.layer_norm(torch.randn(B, 77, 1024, generator=g), (1024,)).cuda()
    uc = torch.nn.functional.layer_norm(torch.randn(B, 77, 1024, generator=g), (1024,)).cuda()
    return g, c, uc


def _timed(f, rounds):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def ddim_steps(rounds=3):
    """ms per step of the 100-step DDIM loop alone (sample_latents), unguided and guided, after two warm-up calls each."""
    g, c, uc = _cond()
    x = torch.randn(B, 4, 10, 78, generator=g).cuda()
    out = []
    for guided in (False, True):
        m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, precision="bf16x3")
        m.ctx.set_concurrency(1)
        f = (lambda: m.sample_latents(x, c, uc, SCALE, S)) if guided else (lambda: m.sample_latents(x, c, None, 1.0, S))
        f()
        f()
        out.append(1e3 * statistics.mean(_timed(f, rounds)) / S)
        m.close()
    return out


def bench_ab(parent, steps):
    """The DDIM regression check (the loops share csrc/ddim.cpp's Loop): `python bench.py --gpus 1 --steps N` for this build and for
    the parent checkout, twice each, alternated, one process at a time.  The new build's mean may not be lower than the parent's
    by more than the parent's own spread between its two runs."""
    import json
    flags = ["--gpus", "1", "--steps", str(steps), "--warmup", "2", "--no-secondary", "--no-cpu-baseline", "--no-roofline"]
    head = ["DDIM regression check: python bench.py %s (audio-seconds/s; parent, new, parent, new in this order)" % " ".join(flags)]
    if not parent:
        return head + ["  NOT MEASURED (no PARENT checkout given)"]
    vals = {"parent": [], "new": []}
    for _ in range(2):
        for who, cwd in (("parent", parent), ("new", ".")):
            r = subprocess.run([sys.executable, "bench.py"] + flags, cwd=cwd, capture_output=True, text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"value"' in ln]
            if r.returncode != 0 or not line:
                return head + ["  NOT MEASURED: bench.py of the %s build failed (%s)"
                               % (who, (r.stderr.strip().splitlines() or ["no output"])[-1][:160])]
            vals[who].append(float(json.loads(line[-1])["value"]))
    p, n = vals["parent"], vals["new"]
    spread = abs(p[0] - p[1])
    d = statistics.mean(n) - statistics.mean(p)
    return head + ["  parent %.2f %.2f  (mean %.2f, spread %.2f)" % (p[0], p[1], statistics.mean(p), spread),
                   "  new    %.2f %.2f  (mean %.2f)" % (n[0], n[1], statistics.mean(n)),
                   "  new - parent = %+.2f: %s" % (d, "not lower than the parent by more than the parent's spread" if d >= -spread
                                                   else "LOWER than the parent by more than the parent's own spread")]


def main():
    args = [a for a in sys.argv[1:]]
    if args and args[0] == "--ddim-steps":
        print("ddim_ms_per_step unguided %.4f guided %.4f" % tuple(ddim_steps()))
        return
    out_path = args[0] if len(args) > 0 else "profiles/ddpm_timing.txt"
    rounds = int(args[1]) if len(args) > 1 else 3
    parent = args[2] if len(args) > 2 else None
    bench_steps = int(args[3]) if len(args) > 3 else 6
    from audiogpt_amd.ldm.ddpm import schedule_buffers
    g, c, uc = _cond()
    x = torch.randn(B, 4, 10, 78, generator=g).cuda()
    runs = {}
    for name, f_of in (("a_ddpm_unguided_1000", lambda m: (lambda: m.generate(x, c, sampler="ddpm"))),
                       ("b_ddpm_guided_1000", lambda m: (lambda: m.generate(x, c, uc, SCALE, sampler="ddpm"))),
                       ("c_ddim_guided_100", lambda m: (lambda: m.generate(x, c, uc, SCALE, S)))):
        m = MakeAnAudio("cuda:0", ldm=C.LDM_T2A, vocoder_cfg=C.HIFIGAN_16K, precision="bf16x3")
        m.ctx.set_concurrency(1)
        f = f_of(m)
        f()
        f()
        runs[name] = (m, f)
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, (m, f) in runs.items():
            times[k] += _timed(f, 1)
    audio = runs["c_ddim_guided_100"][0].audio_seconds(B, 8 * 78)
    steps = {"a_ddpm_unguided_1000": T, "b_ddpm_guided_1000": T, "c_ddim_guided_100": S}
    text = ["ancestral (DDPM) sampling: generate at 8 T2A prompts, one MI355X, all runs in one process", "",
            "command: python scripts/ddpm_timing.py  (%d timed rounds after 2 warm-up calls each, runs alternated)" % rounds,
            "shapes:  latent [8, 4, 10, 78], 77-token conditioning, bf16x3, hipGraph on, set_concurrency(1); guided = CFG 1.5 (two",
            "         lanes); a and b draw their 1000 x [8, 4, 10, 78] step noise (100 MB) inside the call; VAE decode and HiFi-GAN included",
            "", "%-22s %8s %10s %10s %12s %16s" % ("run", "audio s", "mean s", "sd s", "ms / step", "audio-seconds/s")]
    for k, v in times.items():
        mean = statistics.mean(v)
        text.append("%-22s %8.1f %10.4f %10.4f %12.4f %16.2f" % (k, audio, mean, statistics.stdev(v) if len(v) > 1 else 0.0,
                                                                1e3 * mean / steps[k], audio / mean))
    # the device loops alone, per step: ancestral over fixed noise against this build's own DDIM loop
    tabs = schedule_buffers(T, C.LDM_T2A["linear_start"], C.LDM_T2A["linear_end"])
    noise = torch.randn(T, B, 4, 10, 78, device="cuda")
    loop = {}
    for name, key, kw in (("ancestral unguided", "a_ddpm_unguided_1000", dict(cond=c)),
                          ("ancestral guided", "b_ddpm_guided_1000", dict(cond=c, uncond=uc, scale=SCALE))):
        m = runs[key][0]
        f = lambda m=m, kw=kw: m.unet.ddpm_sample(x, tabs, T, noise_p=noise, **kw)
        f()
        loop[name] = [1e3 * t / T for t in _timed(f, rounds)]
    own = ddim_steps(rounds)
    text += ["", "device loops alone, ms per step (mean of %d calls; ancestral: UNet.ddpm_sample over fixed noise, 1000 steps; DDIM:" % rounds,
             "sample_latents, 100 steps):",
             "  %-28s %8.4f   (calls: %s)" % ("ancestral unguided", statistics.mean(loop["ancestral unguided"]),
                                             " ".join("%.4f" % t for t in loop["ancestral unguided"])),
             "  %-28s %8.4f   (calls: %s)" % ("ancestral guided", statistics.mean(loop["ancestral guided"]),
                                             " ".join("%.4f" % t for t in loop["ancestral guided"])),
             "  %-28s %8.4f" % ("this build's DDIM unguided", own[0]), "  %-28s %8.4f" % ("this build's DDIM guided", own[1])]
    slower = []
    if not parent:
        text.append("  parent commit's DDIM yardstick: NOT MEASURED (no PARENT checkout given): the ancestral steps above are unjudged")
    else:
        got = []
        for _ in range(2):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--ddim-steps"], cwd=parent, capture_output=True, text=True,
                               timeout=600)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("ddim_ms_per_step")]
            if r.returncode != 0 or not line:
                text.append("  parent commit's DDIM yardstick: NOT MEASURED (%s): the ancestral steps above are unjudged"
                            % (r.stderr.strip().splitlines() or ["no output"])[-1][:160])
                break
            w = line[0].split()
            got.append((float(w[2]), float(w[4])))
        if len(got) == 2:
            for i, name in enumerate(("unguided", "guided")):
                p = [got[0][i], got[1][i]]
                spread = abs(p[0] - p[1])
                mine = statistics.mean(loop["ancestral " + name])
                d = mine - statistics.mean(p)
                if d > 2 * spread:
                    slower.append(name)
                text.append("  parent commit's DDIM %-9s %8.4f %8.4f  (two runs; spread %.4f)   ancestral - parent = %+.4f ms: %s"
                            % (name, p[0], p[1], spread, d,
                               "within twice the spread" if d <= 2 * spread else "SLOWER than the parent by more than twice the spread"))
    # the step kernel's share: eager 10-step chain under the per-kernel timer
    m = runs["b_ddpm_guided_1000"][0]
    kw = dict(cond=c, uncond=uc, scale=SCALE, noise_p=noise[:10], use_graph=False)
    m.unet.ddpm_sample(x, tabs, 10, **kw)
    m.ctx.prof_begin()
    m.unet.ddpm_sample(x, tabs, 10, **kw)
    rows = m.ctx.prof_end()
    total = sum(r["ms"] for r in rows.values())
    text += ["", "eager 10-step guided chain under the per-kernel timer (sum of launch durations %.2f ms)%s:"
             % (total, "; the %s ancestral step is slower than the parent's DDIM step by more than twice the spread -- this table shows "
                "where a step's time goes" % " and the ".join(slower) if slower else "")]
    for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:12]:
        text.append("  %-40s %5d launches %9.3f ms  %6.3f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
    for k in rows:
        if k.startswith("ddpm_step_kernel") or k.startswith("ddim_prepare_kernel"):
            text.append("  -> %-37s %5d launches %9.3f ms  %6.3f %% of the launches' time"
                        % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
    for m, _ in runs.values():
        m.close()
    del runs, noise
    torch.cuda.empty_cache()
    text += [""] + bench_ab(parent, bench_steps)
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
