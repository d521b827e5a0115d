"""CPU checks of the FastSpeech2MIDI work: the host restatement (tests/fs2_ref.py) against the reference's own outputs
(tests/golden/fs2_*.npz, written by tests/golden/make_golden_fs2.py), the state-dict key layout, the masked-attention
reference's own edge cases, the C ABI entries, every refusal with its reason, the host checks of the integer inputs, and the
register metadata of the new kernels."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import attn_ref as A
from tests import fs2_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audiogpt_amd", "csrc")
ENTRIES = ("maa_fs2_create", "maa_fs2_destroy", "maa_fs2_encode", "maa_fs2_length_regulate", "maa_fs2_decode",
           "maa_op_attention_masked")


@pytest.mark.parametrize("name,prefix", R.CASES)
def test_restatement_matches_reference(name, prefix):
    """Gate: 10 x the reference's own fp32 - fp64 difference of the tensor (recorded by the generator), relative to
    max|reference|; the integers exactly."""
    cfg, sd, g = R.load_case(name, prefix)
    inp = R.inputs(g)
    with torch.no_grad():
        got = R.forward(sd, cfg, **inp)
        got64 = R.forward(sd, cfg, dtype=torch.float64, **inp)
    for what in R.FLOATS:
        ref, floor = torch.from_numpy(g[what]), float(g["floor_" + what])
        scale = float(ref.abs().max())
        err = float((got[what] - ref).abs().max())
        err64 = float((got64[what] - ref.double()).abs().max())
        print("%s%s %s: fp32 restatement %.2e, fp64 restatement %.2e, recorded floor %.2e, max|ref| %.2f" % (name, prefix, what, err, err64, floor, scale))
        assert floor > 0
        assert err / scale <= 10 * floor / scale, (what, err, floor)
        assert err64 / scale <= 10 * floor / scale, (what, err64, floor)
    for r in (got, got64):
        assert torch.equal(r["mel2ph"], torch.from_numpy(g["mel2ph"]))
        if "dur_choice" in g:
            assert torch.equal(r["dur_choice"], torch.from_numpy(g["dur_choice"]))
    # padding rows are exactly 0
    pad = inp["txt_tokens"] == 0
    assert bool((got["encoder_out"][pad] == 0).all())
    off = torch.from_numpy(g["mel2ph"]) == 0
    assert bool((got["decoder_inp"][off] == 0).all()) and bool((got["mel_out"][off] == 0).all())


def test_golden_cases_are_what_the_tests_need():
    _, _, g = R.load_case("fs2_b2_t33")
    tot = (torch.from_numpy(g["mel2ph"]) > 0).sum(-1)
    assert g["mel2ph"].shape[1] > 128 and int(tot.max() - tot.min()) >= 64          # a second query tile; key tiles hidden for one sample
    assert int((g["txt_tokens"][0] == 0).sum()) == 1 and int((g["txt_tokens"][1] != 0).sum()) == 20
    live = g["txt_tokens"] != 0
    assert 3 <= float(torch.from_numpy(g["dur_choice"])[torch.from_numpy(live)].float().median()) <= 5
    for p in ("t1.", "t4."):
        _, _, s = R.load_case("fs2_short", p)
        assert s["mel2ph"].shape[1] < 9
    _, _, m = R.load_case("fs2_given_mel2ph")
    assert m["mel2ph_in"].shape == (2, 70) and "dur_choice" not in m
    z = (torch.from_numpy(m["mel2ph_in"]) == 0).sum(-1)
    assert int(z[0]) != int(z[1]) and 6 not in m["mel2ph_in"][0].tolist()              # token 5 (1-based 6) has no frame
    wcfg, _, w = R.load_case("fs2_ph384_b2_t9")
    assert wcfg["predictor_hidden"] == 384 and wcfg["hidden_size"] == 256            # the duration head leaves one float4 per lane
    assert w["txt_tokens"].shape == (2, 9) and (w["txt_tokens"][0] != 0).all() and (w["txt_tokens"][1] == 0).tolist() == [False] * 6 + [True] * 3


def test_state_dict_keys_match_reference():
    for name in sorted({n for n, _ in R.CASES}):
        cfg, sd, g = R.load_case(name)
        assert list(sd.keys()) == g["keys"], name
    sd = WT.make_fs2_state_dict(C.FASTSPEECH2_MIDI)
    assert len(sd) == 116
    assert sd["encoder_embed_tokens.weight"] is sd["encoder.embed_tokens.weight"]
    assert bool((sd["encoder.embed_tokens.weight"][0] == 0).all()) and bool((sd["midi_embed.weight"][0] == 0).all())
    for p in ("encoder.layers.0.op.layer_norm1.", "decoder.layers.3.op.layer_norm2.", "encoder.layer_norm.", "dur_predictor.conv.4.3."):
        assert float((sd[p + "weight"] - 1).abs().max()) > 0.05 and float(sd[p + "bias"].abs().max()) > 0.05
    assert float(sd["decoder.pos_embed_alpha"]) != 1.0
    assert tuple(sd["decoder.embed_positions._float_tensor"].shape) == (1,)


def test_rel_pos_table_is_reversed():
    tab = R.rel_pos_table(3, 8)
    div = math.exp(2 * -(math.log(10000.0) / 8))
    assert float(tab[0, 0]) == pytest.approx(math.sin(4999.0), abs=1e-3) and float(tab[2, 1]) == pytest.approx(math.cos(4997.0), abs=1e-3)
    assert float(tab[1, 2]) == pytest.approx(math.sin(4998.0 * div), abs=1e-3)


def test_masked_attention_reference_edges():
    """The float64 yardstick itself: zero weight on hidden keys whatever their logit, and the sharp case's error scale."""
    alpha = R.OP_DH ** -0.5
    q, k, v, hidden = R.sharp_hidden_qkv(1, R.OP_HEADS, R.OP_DH, 70, alpha, 5)
    ref = R.masked_attention_ref(q, k, v, R.OP_HEADS, alpha, hidden)
    assert float(ref.min()) > 0                                             # only the positive (even) rows of v are visible
    unmasked = A.attention_ref(q, k, v, R.OP_HEADS, alpha)
    assert A.rel_max(unmasked, ref) > 0.5                                   # admitting the hidden keys is an error of the range
    k2, v2 = k.clone(), v.clone()
    k2[:, hidden[0]] = 1e3
    v2[:, hidden[0]] = -1e6
    assert torch.equal(R.masked_attention_ref(q, k2, v2, R.OP_HEADS, alpha, hidden), ref)
    for N, B, case in R.OP_SHAPES:
        h = R.op_hidden(B, N, case)
        assert bool((~h).any(dim=1).all()), case                            # every sample keeps a visible key


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _backend_cfg(cfg):
    from audiogpt_amd import backend
    return backend.fs2_config(cfg)


def test_abi_entries_are_declared_bound_and_reject_null(lib):
    from audiogpt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")), name
    h = ctypes.c_void_p()
    assert lib.maa_fs2_create(None, None, None, 0, ctypes.byref(h)) < 0
    assert b"null" in lib.maa_last_error()
    cfg = _backend_cfg(C.FASTSPEECH2_MIDI)
    assert lib.maa_fs2_create(None, ctypes.byref(cfg), None, 0, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0      # no context
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_encode(None, None, None, None, None, None, 1, 1, None, None, None, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_length_regulate(None, None, None, 1, 1, 1, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_decode(None, None, None, None, 1, 1, 1, None, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_op_attention_masked(None, None, 128, 128, None, 128, 128, None, 128, 128, 1, 1, 128, 1, 1, 1.0, None, 128, 0, 0, None) < 0
    assert len(lib.maa_last_error()) > 0
    assert lib.maa_fs2_destroy(None) == 0


REFUSALS = [(dict(use_pitch_embed=True), "use_pitch_embed"), (dict(use_energy_embed=True), "use_energy_embed"),
            (dict(use_spk_id=True), "use_spk_id"), (dict(use_spk_embed=True), "use_spk_embed"), (dict(use_bert=True), "use_bert"),
            (dict(rel_pos=False), "rel_pos"), (dict(use_pos_embed=False), "use_pos_embed"), (dict(ffn_padding="LEFT"), "SAME"),
            (dict(ffn_act="relu"), "gelu"), (dict(dur_loss="crf"), "mse"), (dict(encoder_type="conformer"), "encoder_type"),
            (dict(decoder_type="conv"), "decoder_type"), (dict(num_heads=4), "128"), (dict(hidden_size=384), "128")]
# the library's own refusal of the same settings: (field, value, reason)
LIB_REFUSALS = [("use_pitch_embed", 1, b"use_pitch_embed"), ("use_energy_embed", 1, b"use_energy_embed"), ("use_spk_id", 1, b"use_spk_id"),
                ("use_spk_embed", 1, b"use_spk_embed"), ("use_bert", 1, b"use_bert"), ("rel_pos", 0, b"rel_pos"),
                ("use_pos_embed", 0, b"use_pos_embed"), ("ffn_padding_same", 0, b"SAME"), ("ffn_act_gelu", 0, b"gelu"),
                ("dur_loss_mse", 0, b"mse"), ("encoder_fft", 0, b"encoder_type"), ("decoder_fft", 0, b"decoder_type"),
                ("num_heads", 4, b"128")]


@pytest.mark.parametrize("change,reason", REFUSALS)
def test_unsupported_configuration_is_refused_with_the_reason(change, reason):
    from audiogpt_amd import _lib
    from audiogpt_amd.diffsinger import FastSpeech2MIDI
    with pytest.raises(_lib.MaaError, match=reason):
        _backend_cfg(dict(C.FASTSPEECH2_MIDI, **change))
    with pytest.raises(_lib.MaaError, match=reason):          # the reference-surface class, before it makes a context
        FastSpeech2MIDI(dict(C.FASTSPEECH2_MIDI, **change))


@pytest.mark.parametrize("field,value,reason", LIB_REFUSALS)
def test_library_refuses_before_touching_a_device(lib, field, value, reason):
    cfg = _backend_cfg(C.FASTSPEECH2_MIDI)
    setattr(cfg, field, value)
    h = ctypes.c_void_p()
    assert lib.maa_fs2_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0
    assert reason in lib.maa_last_error()


def test_integer_inputs_are_checked_on_the_host():
    """_check needs no device: it runs on an object that has only its cfg."""
    from audiogpt_amd.diffsinger import FastSpeech2MIDI
    m = FastSpeech2MIDI.__new__(FastSpeech2MIDI)
    m.cfg = dict(C.FASTSPEECH2_MIDI)
    tok = torch.tensor([[3, 5, 0, 7], [1, 0, 0, 0]])
    midi, slur = torch.full((2, 4), 60), torch.zeros(2, 4, dtype=torch.long)
    m._check(tok, midi, slur, None)
    m._check(tok, midi, None, torch.tensor([[1, 1, 2, 4, 0], [1, 0, 0, 0, 0]]))
    for bad, reason in ((dict(txt_tokens=tok.clone().fill_(64)), "vocab_size"), (dict(txt_tokens=-tok), "vocab_size"),
                        (dict(txt_tokens=torch.tensor([[3, 5, 0, 7], [0, 0, 0, 0]])), "live token"),
                        (dict(pitch_midi=midi + 240), "300"), (dict(pitch_midi=None), "required"), (dict(is_slur=slur + 2), "is_slur"),
                        (dict(mel2ph=torch.tensor([[1, 5], [1, 1]])), "T_txt"), (dict(mel2ph=torch.tensor([[1, 2], [0, 0]])), "all 0"),
                        (dict(mel2ph=torch.tensor([[1, 2]])), "T_mel")):
        kw = dict(txt_tokens=tok, pitch_midi=midi, is_slur=slur, mel2ph=None)
        kw.update(bad)
        with pytest.raises(ValueError, match=reason):
            m._check(**kw)


def test_new_kernels_do_not_spill(tmp_path):
    """vgpr_spill_count and the private segment of every kernel of fs2.hip and of the masked instantiations of flash_attn.hip in
    the cross-compiled gfx950 assembly's metadata (read as tests/test_pe_host.py::test_pitch_kernels_do_not_spill reads it)."""
    from audiogpt_amd.build import FLAGS
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    meta = {}
    for src in ("fs2.hip", "flash_attn.hip"):
        out = str(tmp_path / (src + ".s"))
        cmd = [hipcc] + [f for f in FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                                              os.path.join(CSRC, src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                             r"\s+\.vgpr_spill_count:\s+(\d+)", open(out).read()):
            meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    names = " ".join(meta)
    for k in ("fs2_embed_kernel", "fs2_dur_head_kernelILi1E", "fs2_dur_head_kernelILi2E", "fs2_dur_head_kernelILi4E", "fs2_length_kernel",
              "fs2_expand_kernel",
              "flash_attn_kernelILi128ELi3ELb1E", "flash_attn_kernelILi128ELi1ELb1E"):
        assert k in names, k
    for name, (private, vg, spill) in meta.items():
        assert spill == 0 and private == 0, (name, private, spill)
        if "fs2_" in name:
            assert vg <= 128, (name, vg)          # row kernels: four waves per SIMD
        if "Li128E" in name:
            assert vg <= 512, (name, vg)          # one workgroup of four waves per CU: the whole unified register file of a SIMD
