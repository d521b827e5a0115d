"""What DiffSinger's back end costs per utterance on the device: one PitchExtractor forward at B = 1, T = 1500 frames (8 s at hop
128 / 24 kHz), next to the NSF HiFi-GAN on the same frames and ONE evaluation of the diffusion's denoiser at the same T, all in
one process on one context (bf16x3).

    python scripts/pe_timing.py [OUT=profiles/pe_timing.txt]

Times are the library profiler's (hipEvent pairs around every launch, eager): the sum of a call's launch durations and its rows,
after one warm-up call each.  The extractor runs once per utterance, the denoiser K_step (or K_step / pndm_speedup) times."""
import sys

import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd.backend import Context, DiffNet, PitchExtractor, Vocoder

B, T = 1, 1500


def profiled(ctx, f):
    f()
    ctx.prof_begin()
    f()
    rows = ctx.prof_end()
    return sum(r["ms"] for r in rows.values()), rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/pe_timing.txt"
    ctx = Context("cuda:0", precision="bf16x3")
    g = torch.Generator().manual_seed(1)
    mel = (torch.rand(B, T, 80, generator=g) * 6.0 - 5.0).cuda()
    pe = PitchExtractor(ctx, C.PITCH_EXTRACTOR, WT.make_pe_state_dict(C.PITCH_EXTRACTOR))
    vcfg = C.HIFIGAN_NSF_24K
    voc = Vocoder(ctx, vcfg, WT.make_vocoder_state_dict(vcfg, seed=6))
    dcfg = C.DIFFSINGER_DS1000
    net = DiffNet(ctx, dcfg, WT.make_diffnet_state_dict(dcfg, seed=7))
    hop = voc.hop
    f0 = pe(mel)[1]
    rand_ini, noise = torch.rand(B, 9, device="cuda"), torch.randn(B, T * hop, 9, device="cuda")
    x, cond, t = torch.randn(B, 1, 80, T, device="cuda"), torch.randn(B, 256, T, device="cuda"), torch.full((B,), 500.0, device="cuda")
    parts = [("PitchExtractor.forward", lambda: pe(mel)),
             ("NSF HiFi-GAN forward_f0 (%d samples)" % (T * hop), lambda: voc.forward_f0(mel.transpose(1, 2).contiguous(), f0, rand_ini, noise)),
             ("DiffNet.forward (one denoiser evaluation)", lambda: net(x, t, cond))]
    text = ["DiffSinger back end: device time per call, one MI355X, one process, one context", "",
            "command: python scripts/pe_timing.py",
            "shapes:  B = %d, T = %d frames (%.1f s at hop %d / %d Hz), bf16x3, eager launches under the library's per-launch timer" %
            (B, T, T * hop / vcfg["sampling_rate"], hop, vcfg["sampling_rate"]),
            "         voiced frames in the extractor's f0: %d of %d (seeded random weights)" % (int((f0 > 0).sum()), T), ""]
    for name, f in parts:
        total, rows = profiled(ctx, f)
        text.append("%-48s %8.3f ms  (%d launches)" % (name, total, sum(r["launches"] for r in rows.values())))
        for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:8]:
            text.append("    %-44s %5d launches %9.3f ms  %6.2f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
