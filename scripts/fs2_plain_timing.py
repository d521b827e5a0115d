"""What the plain FastSpeech2 front end costs per utterance on the device, at the shape and in the manner of scripts/fs2_timing.py
(29 phonemes, 1000 frames, B = 1 and B = 8, bf16x3, a caller's mel2ph, everything else predicted): config.FASTSPEECH2 as it is
(pitch branch, no energy, no speakers) and with the energy branch and three speaker tables, next to the e2e FastSpeech2MIDI front
end (encode + decode) timed in the same process.  The variance stage -- what lies between the expand and the decoder: the
broadcast speaker add, the pitch branch, the energy branch with its tail -- is timed alone and its launches are counted.

    python scripts/fs2_plain_timing.py [OUT=profiles/fs2_plain_timing.txt]

Wall times and the per-kernel split are taken as fs2_timing.py takes them (its score() and wall() are used)."""
import os
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fs2_timing as F
from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd.backend import Context, FastSpeech2MIDI, FastSpeech2Plain, FS2Pitch


def is_pitch(k):
    return k.startswith(("pitch_embed.", "pitch_predictor."))


def build(ctx, cfg):
    sd = WT.make_fs2_plain_state_dict(cfg)
    net = FastSpeech2Plain(ctx, dict(cfg, use_pitch_embed=False), {k: v for k, v in sd.items() if not is_pitch(k)})
    pitch = FS2Pitch(ctx, dict(cfg, use_energy_embed=False, use_spk_id=False, use_spk_embed=False),
                     {k: v for k, v in sd.items() if is_pitch(k)})
    return net, pitch


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/fs2_plain_timing.txt"
    ctx = Context("cuda:0", precision="bf16x3")
    plain_cfg = C.FASTSPEECH2
    full_cfg = dict(C.FASTSPEECH2_LIBRITTS, use_energy_embed=True, use_split_spk_id=True)
    models = [("plain (pitch branch)", plain_cfg) + build(ctx, plain_cfg), ("+ energy + speakers", full_cfg) + build(ctx, full_cfg)]
    midi = FastSpeech2MIDI(ctx, C.FASTSPEECH2_MIDI, WT.make_fs2_state_dict(C.FASTSPEECH2_MIDI))
    text = ["Plain FastSpeech2 front end: time per utterance, one MI355X, one process, one context", "",
            "command: python scripts/fs2_plain_timing.py",
            "shapes:  T_txt = %d phonemes, T_mel = %d frames (a caller's mel2ph), bf16x3, eager launches; wall = host clock around %d calls"
            % (F.T_TXT, F.T_MEL, F.REPS),
            "         ending in a stream synchronise, profiler off; the split = the library's per-launch timer in a call of its own", ""]
    for B in (1, 8):
        dev = [t.cuda() for t in F.score(B)]
        tok, m2p = dev[0], dev[4]
        ids = (torch.arange(3 * B).reshape(3, B) * 7 % 2321).cuda()
        for label, cfg, net, pitch in models:
            spk = bool(cfg["use_spk_id"])

            def variance(origin, sp):
                pred_inp = net.add_speaker(origin, sp[2], m2p) if spk else origin
                acc, _, f0 = pitch.forward(origin, m2p, pred_inp=pred_inp if spk else None)
                if spk or cfg["use_energy_embed"]:
                    acc = net.finish(pred_inp, acc, m2p, spk=sp[0] if spk else None)[0]
                return acc, f0

            def front():
                sp = net.speaker(ids=ids) if spk else None
                enc = net.encode(tok, spk_dur=sp[1] if spk else None)[0]
                origin, _ = net.decode(enc, m2p, skip_decoder=True)
                acc, f0 = variance(origin, sp)
                return net.run_decoder(acc, m2p), f0

            sp = net.speaker(ids=ids) if spk else None
            origin = net.decode(net.encode(tok, spk_dur=sp[1] if spk else None)[0], m2p, skip_decoder=True)[0]
            ms = F.wall(ctx.synchronize, front)
            ms_var = F.wall(ctx.synchronize, lambda: variance(origin, sp))
            front()
            ctx.prof_begin()
            front()
            rows = ctx.prof_end()
            ctx.prof_begin()
            variance(origin, sp)
            var_rows = ctx.prof_end()
            total = sum(r["ms"] for r in rows.values())
            text.append("%-22s B = %d   wall %8.3f ms   device %8.3f ms  (%d launches)"
                        % (label, B, ms, total, sum(r["launches"] for r in rows.values())))
            for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:8]:
                text.append("    %-44s %5d launches %9.3f ms  %6.2f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
            text.append("    the variance stage alone                     %5d launches   wall %8.3f ms"
                        % (sum(r["launches"] for r in var_rows.values()), ms_var))
        ms_e2e = F.wall(ctx.synchronize, lambda: midi.decode(midi.encode(dev[0], dev[1], dev[2], dev[3])[0], m2p))
        text.append("the e2e MIDI front end (encode + decode), same process, B = %d    wall %8.3f ms   (profiles/fs2_timing.txt)" % (B, ms_e2e))
        text.append("")
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
