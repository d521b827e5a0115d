"""What the cascade front end costs per utterance on the device: FastSpeech2MIDI encode + decode without the decoder + the pitch
branch (FS2Pitch) + run_decoder, at the shape and in the manner of scripts/fs2_timing.py (29 phonemes, 1000 frames, B = 1 and
B = 8, bf16x3, a caller's mel2ph, pitch and voicing predicted), next to the e2e front end (encode + decode) timed in the same
process, and the pitch branch alone.

    python scripts/fs2_cascade_timing.py [OUT=profiles/fs2_cascade_timing.txt]

Wall times and the per-kernel split are taken as fs2_timing.py takes them (its score() and wall() are used)."""
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fs2_timing as F
from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd.backend import Context, FastSpeech2MIDI, FS2Pitch


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/fs2_cascade_timing.txt"
    ctx = Context("cuda:0", precision="bf16x3")
    cfg = C.FASTSPEECH2_MIDI_CASCADE
    sd = WT.make_fs2_state_dict(cfg)
    is_pitch = lambda k: k.startswith(("pitch_embed.", "pitch_predictor."))      # noqa: E731
    net = FastSpeech2MIDI(ctx, dict(cfg, use_pitch_embed=False), {k: v for k, v in sd.items() if not is_pitch(k)})
    pitch = FS2Pitch(ctx, cfg, {k: v for k, v in sd.items() if is_pitch(k)})
    text = ["DiffSinger cascade front end: time per utterance, one MI355X, one process, one context", "",
            "command: python scripts/fs2_cascade_timing.py",
            "shapes:  T_txt = %d phonemes, T_mel = %d frames (a caller's mel2ph), bf16x3, eager launches; wall = host clock around %d calls"
            % (F.T_TXT, F.T_MEL, F.REPS),
            "         ending in a stream synchronise, profiler off; the split = the library's per-launch timer in a call of its own", ""]
    for B in (1, 8):
        dev = [t.cuda() for t in F.score(B)]

        def e2e():
            return net.decode(net.encode(dev[0], dev[1], dev[2], dev[3])[0], dev[4])

        def cascade():
            enc = net.encode(dev[0], dev[1], dev[2], dev[3])[0]
            origin, _ = net.decode(enc, dev[4], skip_decoder=True)
            dec_inp, pitch_pred, f0 = pitch.forward(origin, dev[4])
            return net.run_decoder(dec_inp, dev[4]), f0

        origin = net.decode(net.encode(dev[0], dev[1], dev[2], dev[3])[0], dev[4], skip_decoder=True)[0]
        ms = F.wall(ctx.synchronize, cascade)
        ms_e2e = F.wall(ctx.synchronize, e2e)
        ms_pitch = F.wall(ctx.synchronize, lambda: pitch.forward(origin, dev[4]))
        cascade()
        ctx.prof_begin()
        cascade()
        rows = ctx.prof_end()
        total = sum(r["ms"] for r in rows.values())
        text.append("encode + decode (no decoder) + pitch + run_decoder, B = %d   wall %8.3f ms   device %8.3f ms  (%d launches)"
                    % (B, ms, total, sum(r["launches"] for r in rows.values())))
        for k in sorted(rows, key=lambda k: -rows[k]["ms"])[:10]:
            text.append("    %-44s %5d launches %9.3f ms  %6.2f %%" % (k, rows[k]["launches"], rows[k]["ms"], 100.0 * rows[k]["ms"] / total))
        text.append("the pitch branch alone (FS2Pitch.forward), B = %d            wall %8.3f ms" % (B, ms_pitch))
        text.append("the e2e front end (encode + decode), same process, B = %d    wall %8.3f ms   (profiles/fs2_timing.txt)" % (B, ms_e2e))
        text.append("")
    text = "\n".join(text) + "\n"
    print(text)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
