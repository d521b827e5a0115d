"""CPU checks of the FastSpeech2MIDI pitch branch (the cascade singing configurations): the C ABI entries and the new structure
against the header, every refusal with its reason, the state-dict key layout, the float32 restatement of the pitch tail
(tests/fs2_pitch_ref.py) against the reference's own outputs (tests/golden/fs2_pitch_*.npz, written by
tests/golden/make_golden_fs2_pitch.py), the generator's own conditions, and the register metadata of the new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import fs2_pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audiogpt_amd", "csrc")
ENTRIES = ("maa_fs2_run_decoder", "maa_fs2_pitch_create", "maa_fs2_pitch_destroy", "maa_fs2_pitch_forward")
# sha256 of make_fs2_state_dict(C.FASTSPEECH2_MIDI, seed=17) (P.state_dict_hash) on the commit before the pitch keys were added
FS2_SEED17_HASH = "158bb7716b2fe9a67db52d38405db15b83fdec214f2c431467d4d2bda67e2f1a"
GATE = 2e-4          # the bf16x3 gate the generator keeps the logits clear of 0 by


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)


def test_abi_entries_are_declared_bound_and_reject_null(lib):
    from audiogpt_amd import _lib, backend
    src = _header()
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")), name
    h = ctypes.c_void_p()
    cfg = backend.fs2_pitch_config(C.FASTSPEECH2_MIDI_CASCADE)
    assert lib.maa_fs2_pitch_create(None, None, None, 0, ctypes.byref(h)) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_pitch_create(None, ctypes.byref(cfg), None, 0, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_pitch_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0      # no context
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_pitch_forward(None, None, None, None, None, None, 1, 1, None, None, None, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_run_decoder(None, None, None, None, 1, 1, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_fs2_pitch_destroy(None) == 0


def test_bad_sizes_fail_before_the_context_is_touched(lib):
    """Non-null garbage pointers: the size check answers first, nothing is dereferenced."""
    p = ctypes.c_void_p(64)
    for B, T in ((0, 4), (4, 0), (1 << 10, 1 << 10)):
        assert lib.maa_fs2_pitch_forward(p, p, p, p, None, None, B, T, p, p, p, None) < 0
        assert b"B, T_mel" in lib.maa_last_error()
        assert lib.maa_fs2_run_decoder(p, p, p, p, B, T, p) < 0
        assert b"B, T_mel" in lib.maa_last_error()


def test_config_structure_matches_header():
    from audiogpt_amd import _lib
    body = re.search(r"typedef struct maa_fs2_pitch_config \{(.*?)\} maa_fs2_pitch_config;", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int": ctypes.c_int, "float": ctypes.c_float}[ctype]) for n in names.split(",")]
    assert fields == list(_lib.maa_fs2_pitch_config._fields_)
    assert [n for n, _ in fields] == ["hidden_size", "predictor_hidden", "predictor_layers", "predictor_kernel", "ffn_padding_same",
                                      "pitch_type_frame", "pitch_ar", "use_uv", "pitch_norm", "f0_mean", "f0_std"]


def test_cascade_config_is_the_midi_one_with_the_pitch_branch():
    c = C.FASTSPEECH2_MIDI_CASCADE
    assert {k: c[k] for k in C.FASTSPEECH2_MIDI if k != "use_pitch_embed"} == {k: v for k, v in C.FASTSPEECH2_MIDI.items() if k != "use_pitch_embed"}
    assert c["use_pitch_embed"] is True and c["pitch_type"] == "frame" and c["use_uv"] is True and c["pitch_norm"] == "log"
    assert c["pitch_ar"] is False and c["predictor_layers"] == 5 and c["predictor_kernel"] == 5 and (c["f0_mean"], c["f0_std"]) == (0.0, 1.0)
    from audiogpt_amd import backend
    s = backend.fs2_pitch_config(dict(c, pitch_norm="standard", f0_mean=220.0, f0_std=60.0, predictor_hidden=384, use_uv=False))
    assert (s.hidden_size, s.predictor_hidden, s.predictor_layers, s.predictor_kernel) == (256, 384, 5, 5)
    assert (s.ffn_padding_same, s.pitch_type_frame, s.pitch_ar, s.use_uv, s.pitch_norm, s.f0_mean, s.f0_std) == (1, 1, 0, 0, 1, 220.0, 60.0)


REFUSALS = [(dict(pitch_type="ph"), "pitch_type 'ph'"), (dict(pitch_type="cwt"), "cwt_predictor"), (dict(pitch_type="cwt"), "no oracle"),
            (dict(pitch_ar=True), "pitch_ar"), (dict(use_energy_embed=True), "use_energy_embed"), (dict(use_spk_id=True), "use_spk_id"),
            (dict(use_spk_embed=True), "use_spk_embed"), (dict(ffn_padding="LEFT"), "SAME"), (dict(pitch_norm="minmax"), "pitch_norm")]
# the library's own refusal of the same settings: (field, value, reason)
LIB_REFUSALS = [("pitch_type_frame", 0, b"pitch_type"), ("pitch_type_frame", 0, b"cwt_predictor"), ("pitch_ar", 1, b"pitch_ar"),
                ("ffn_padding_same", 0, b"SAME"), ("pitch_norm", 2, b"pitch_norm"), ("predictor_kernel", 4, b"odd"),
                ("predictor_layers", 0, b"predictor_layers"), ("predictor_hidden", 2048, b"1024")]


@pytest.mark.parametrize("change,reason", REFUSALS)
def test_unsupported_configuration_is_refused_with_the_reason(change, reason, monkeypatch):
    from audiogpt_amd import _lib, backend, diffsinger
    with pytest.raises(_lib.MaaError, match=reason):
        backend.fs2_pitch_config(dict(C.FASTSPEECH2_MIDI_CASCADE, **change))

    def no_context(*a, **k):
        raise AssertionError("a context was made before the configuration was refused")
    monkeypatch.setattr(diffsinger, "Context", no_context)
    with pytest.raises(_lib.MaaError, match=reason):          # the reference-surface class, before it makes a context
        diffsinger.FastSpeech2MIDICascade(dict(C.FASTSPEECH2_MIDI_CASCADE, **change))


def test_cascade_class_refuses_what_the_inner_model_refuses(monkeypatch):
    from audiogpt_amd import _lib, diffsinger
    monkeypatch.setattr(diffsinger, "Context", lambda *a, **k: pytest.fail("a context was made"))
    for change, reason in ((dict(rel_pos=False), "rel_pos"), (dict(use_bert=True), "use_bert"), (dict(use_pitch_embed=False), "use_pitch_embed")):
        with pytest.raises(_lib.MaaError, match=reason):
            diffsinger.FastSpeech2MIDICascade(dict(C.FASTSPEECH2_MIDI_CASCADE, **change))


@pytest.mark.parametrize("field,value,reason", LIB_REFUSALS)
def test_library_refuses_before_touching_a_device(lib, field, value, reason):
    from audiogpt_amd import backend
    cfg = backend.fs2_pitch_config(C.FASTSPEECH2_MIDI_CASCADE)
    setattr(cfg, field, value)
    h = ctypes.c_void_p()
    assert lib.maa_fs2_pitch_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0
    assert reason in lib.maa_last_error()


def test_state_dict_keys_match_reference_and_the_midi_dict_is_unchanged():
    for name in sorted({n for n, _ in P.CASES}):
        cfg, sd, g = P.load_case(name)
        assert set(sd.keys()) == set(g["keys"]), name
        assert list(sd.keys()) == g["keys"], name          # and in state_dict()'s order
    sd = WT.make_fs2_state_dict(C.FASTSPEECH2_MIDI_CASCADE)
    assert len(sd) == 116 + 25
    H = C.FASTSPEECH2_MIDI_CASCADE["hidden_size"]
    assert tuple(sd["pitch_embed.weight"].shape) == (300, H) and bool((sd["pitch_embed.weight"][0] == 0).all())
    assert tuple(sd["pitch_predictor.linear.weight"].shape) == (2, H) and tuple(sd["pitch_predictor.conv.0.1.weight"].shape) == (H, H, 5)
    assert float(sd["pitch_predictor.pos_embed_alpha"]) != 1.0
    assert float((sd["pitch_predictor.conv.4.3.weight"] - 1).abs().max()) > 0.05 and float(sd["pitch_predictor.conv.4.3.bias"].abs().max()) > 0.05
    # the tensors outside the pitch branch do not depend on it: the committed fs2_*.npz goldens rest on seed 17's
    old = WT.make_fs2_state_dict(C.FASTSPEECH2_MIDI, seed=17)
    assert P.state_dict_hash(old) == FS2_SEED17_HASH
    assert list(old) == [k for k in sd if not k.startswith(("pitch_embed.", "pitch_predictor."))]
    assert all(torch.equal(old[k], sd[k]) for k in old)
    for seed in (3, 17):
        for cfg in (C.FASTSPEECH2_MIDI, dict(C.FASTSPEECH2_MIDI, predictor_hidden=384, enc_layers=1, dec_layers=1)):
            a, b = WT.make_fs2_state_dict(cfg, seed=seed), WT.make_fs2_state_dict(dict(cfg, use_pitch_embed=True), seed=seed)
            assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name,prefix", P.CASES)
def test_tail_restatement_matches_reference(name, prefix):
    """From the golden's pitch_pred and decoder_inp_origin: coarse exactly on unflagged frames, f0_denorm and decoder_inp to
    4 x the reference's own fp32 - fp64 difference (recorded by the generator)."""
    cfg, sd, g = P.load_case(name, prefix)
    t = lambda k: torch.from_numpy(g[k]) if k in g else None      # noqa: E731
    f0_in = t("f0_in")
    before = None if f0_in is None else f0_in.clone()
    f, coarse, dec = P.tail(cfg, t("pitch_pred"), t("decoder_inp_origin"), t("mel2ph"), sd["pitch_embed.weight"], f0=f0_in, uv=t("uv_in"))
    assert before is None or torch.equal(f0_in, before)
    fl = t("flagged")
    assert torch.equal(coarse[~fl], t("coarse")[~fl])
    assert int((coarse - t("coarse")).abs().max()) <= 1
    ff, fd = float(g["floor_f0_denorm"]), float(g["floor_decoder_inp"])
    ef = float((f - t("f0_denorm")).abs().max())
    rows = coarse == t("coarse")
    ed = float((dec - t("decoder_inp"))[rows].abs().max())
    print("%s%s: f0_denorm %.2e (floor %.2e), decoder_inp %.2e (floor %.2e), flagged %d, bins differing %d" % (
        name, prefix, ef, ff, ed, fd, int(fl.sum()), int((~rows).sum())))
    assert ff > 0 and fd > 0
    assert ef <= 4 * ff and ed <= 4 * fd
    pad = t("mel2ph") == 0
    assert bool((f[pad] == 0).all()) and bool((coarse[pad] == 1).all()) and bool((dec[pad] == 0).all())
    if name in P.GIVEN_F0:
        assert not bool(fl.any()) and torch.equal(coarse, t("coarse"))


def test_golden_cases_are_what_the_tests_need():
    for name, prefix in P.CASES:
        cfg, _, g = P.load_case(name, prefix)
        live = g["mel2ph"] > 0
        assert g["flagged"].sum() <= 0.3 * live.sum(), name
        assert not g["flagged"][~live].any()
        if "uv_in" not in g:          # predicted voicing: every live logit clear of 0 by the bf16x3 gate
            assert (np.abs(g["pitch_pred"][..., 1][live]) > GATE * np.abs(g["pitch_pred"]).max()).all(), name
        if "f0_in" not in g:          # the reference zeroed the predicted value on padding frames, through the view
            assert (g["pitch_pred"][..., 0][~live] == 0).all()
        assert (g["f0_denorm"][~live] == 0).all() and (g["coarse"][~live] == 1).all()
        assert g["coarse"].min() >= 1 and g["coarse"].max() <= 255
    _, _, g = P.load_case("fs2_pitch_b2_t33")
    live = g["mel2ph"] > 0
    tot = live.sum(-1)
    assert g["mel2ph"].shape[1] > 128 and int(tot.max() - tot.min()) >= 64
    assert len(np.unique(g["coarse"][live])) >= 20 and g["flagged"].any()
    unv = g["pitch_pred"][..., 1][live] > 0
    assert 0.2 <= unv.mean() <= 0.4 and "dur_choice" in g and "f0_in" not in g
    from tests import fs2_ref as R
    _, _, old = R.load_case("fs2_b2_t33")
    assert all(np.array_equal(g[k], old[k]) for k in ("txt_tokens", "pitch_midi", "midi_dur", "is_slur", "mel2ph", "dur_choice"))
    for name in ("fs2_pitch_given_f0_uv", "fs2_pitch_given_f0"):
        _, _, m = P.load_case(name)
        assert m["mel2ph_in"].shape == (2, 70) and (m["mel2ph_in"] > 0).sum(-1).tolist() == [66, 40] and "dur_choice" not in m
        assert ("uv_in" in m) == name.endswith("_uv")
        hz = 2.0 ** m["f0_in"][0, :6].astype(np.float64)
        assert hz[0] < 50.0 and hz[5] > 1100.0
        if "uv_in" in m:          # (the head of each sample is voiced there: below f0_min, bins 1 / 2, 254 / 255, above f0_max)
            assert m["coarse"][0, :6].tolist() == [1, 1, 2, 254, 255, 255]
    _, _, m2 = P.load_case("fs2_pitch_given_f0_uv")
    assert np.array_equal(m["f0_in"], m2["f0_in"]) and np.array_equal(m["txt_tokens"], m2["txt_tokens"])
    voiced = (m["mel2ph"] > 0) & (m["pitch_pred"][..., 1] <= 0)
    assert voiced.any() and (~voiced & (m["mel2ph"] > 0)).any()
    for p in ("t1.", "t4."):
        _, _, s = P.load_case("fs2_pitch_short", p)
        assert s["mel2ph"].shape[1] < 9
    wcfg, _, w = P.load_case("fs2_pitch_ph384_b2_t9")
    assert wcfg["predictor_hidden"] == 384 and wcfg["predictor_layers"] == 2 and wcfg["enc_layers"] == wcfg["dec_layers"] == 1
    scfg, _, s = P.load_case("fs2_pitch_standard")
    assert (scfg["pitch_norm"], scfg["f0_mean"], scfg["f0_std"]) == ("standard", 220.0, 60.0) and "f0_in" in s and "uv_in" in s


def test_new_kernels_do_not_spill(tmp_path):
    """vgpr_spill_count and the private segment of the pitch tail's three instantiations and the mask kernel in the cross-compiled
    gfx950 assembly's metadata (read as tests/test_fs2_host.py::test_new_kernels_do_not_spill reads it)."""
    from audiogpt_amd.build import FLAGS
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path / "fs2.s")
    cmd = [hipcc] + [f for f in FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                                          os.path.join(CSRC, "fs2.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", open(out).read()):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    new = {k: v for k, v in meta.items() if "fs2_pitch_tail_kernel" in k or "fs2_tgt_mask_kernel" in k}
    names = " ".join(new)
    for k in ("fs2_pitch_tail_kernelILi1E", "fs2_pitch_tail_kernelILi2E", "fs2_pitch_tail_kernelILi4E", "fs2_tgt_mask_kernel"):
        assert k in names, k
    for name, (private, vg, spill) in new.items():
        print(name, "vgprs", vg)
        assert spill == 0 and private == 0, (name, private, spill)
        assert vg <= 128, (name, vg)          # row kernels: four waves per SIMD
