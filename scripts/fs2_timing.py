"""What DiffSinger's front end costs per utterance on the device: FastSpeech2MIDI encode + decode for the utterance of
NeuralSeq/inference/svs/ds_e2e.py's example (29 phonemes, about 1000 frames) at B = 1 and B = 8, next to (a) the host restatement
of the same network (tests/fs2_ref.py, torch on this box's CPU threads) and (b) the diffusion chain the front end feeds under
ds1000 (100 PLMS steps) at B = 1, all in one process on one context (bf16x3).

    python scripts/fs2_timing.py [OUT=profiles/fs2_timing.txt]

Wall times are a host clock around REPS calls that end in a stream synchronise, after a warm-up call, profiler off; the
per-kernel split is the library profiler's (hipEvent pairs around every launch, eager) in a call of its own.  mel2ph is the
caller's here, so that the frame count is the example's and not what random weights predict: the timed front end is encode +
decode, without the length regulator's launch and the read of the B totals between them."""
import sys
import time

import torch

sys.path.insert(0, ".")
from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd.backend import Context, FastSpeech2MIDI
from audiogpt_amd.diffsinger import GaussianDiffusion
from tests import fs2_ref as R

T_TXT, T_MEL, REPS = 29, 1000, 20


def score(B):
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(1, C.FASTSPEECH2_MIDI["vocab_size"], (B, T_TXT), generator=g)
    midi = torch.randint(40, 90, (B, T_TXT), generator=g)
    dur = torch.rand(B, T_TXT, generator=g) * 0.9 + 0.1
    slur = torch.randint(0, 2, (B, T_TXT), generator=g)
    frames = torch.full((T_TXT,), T_MEL // T_TXT)
    frames[: T_MEL - int(frames.sum())] += 1
    mel2ph = torch.repeat_interleave(torch.arange(1, T_TXT + 1), frames)[None].repeat(B, 1)
    return tok, midi, dur, slur, mel2ph


def wall(sync, f, reps=REPS):
    f()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/fs2_timing.txt"
    ctx = Context("cuda:0", precision="bf16x3")
    cfg = C.FASTSPEECH2_MIDI
    sd = WT.make_fs2_state_dict(cfg)
    net = FastSpeech2MIDI(ctx, cfg, sd)
    text = ["DiffSinger front end: time per utterance, one MI355X, one process, one context", "",
            "command: python scripts/fs2_timing.py",
            "shapes:  T_txt = %d phonemes, T_mel = %d frames (a caller's mel2ph), bf16x3, eager launches; wall = host clock around %d calls"
            % (T_TXT, T_MEL, REPS),
            "         ending in a stream synchronise, profiler off; the split = the library's per-launch timer in a call of its own", ""]
    for B in (1, 8):
        tok, midi, dur, slur, mel2ph = score(B)
        dev = [t.cuda() for t in (tok, midi, dur, slur, mel2ph)]

        def front():
            enc = net.encode(dev[0], dev[1], dev[2], dev[3])[0]
            return net.decode(enc, dev[4])

        ms = wall(ctx.synchronize, front)
        front()
        ctx.prof_begin()
        front()
        rows = ctx.prof_end()
        total = sum(r["ms"] for r in rows.values())
        text.append("FastSpeech2MIDI encode + decode, B = %d               wall %8.3f ms   device %8.3f ms  (%d launches)"
                    % (B, ms, total, sum(r["launches"] for r in rows.values())))
        for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:10]:
            text.append("    %-44s %5d launches %9.3f ms  %6.2f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
        with torch.no_grad():
            host = wall(lambda: None, lambda: R.forward(sd, cfg, tok, midi, dur, slur, mel2ph=mel2ph), reps=3)
        text.append("(a) host restatement (torch, %d CPU threads), B = %d   wall %8.3f ms" % (torch.get_num_threads(), B, host))
        text.append("")
    dcfg = C.DIFFSINGER_DS1000
    gd = GaussianDiffusion(dcfg, ctx=ctx)
    tok, midi, dur, slur, mel2ph = score(1)
    dec_inp, mel = net.decode(net.encode(tok, midi, dur, slur)[0], mel2ph)
    cond = dec_inp.transpose(1, 2).contiguous()
    chain = wall(ctx.synchronize, lambda: gd.infer(mel, cond), reps=3)
    text.append("(b) GaussianDiffusion.infer under ds1000 (K_step %d / pndm_speedup %d = %d PLMS steps), B = 1, T = %d   wall %8.3f ms"
                % (dcfg["K_step"], dcfg["pndm_speedup"], dcfg["K_step"] // dcfg["pndm_speedup"], T_MEL, chain))
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
