"""The plain FastSpeech2 (energy branch, speaker embeddings, token-counted positions) without a device: the C ABI's structure and
refusals, the seeded state dict's layout, the goldens' own conditions, and a float32 restatement of the new arithmetic held
against the goldens of the reference's own class (tests/golden/make_golden_fs2_plain.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import fs2_plain_ref as R
from tests import fs2_pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_FIELDS = ["vocab_size", "hidden_size", "enc_layers", "dec_layers", "num_heads", "enc_ffn_kernel_size", "dec_ffn_kernel_size",
              "dur_predictor_layers", "dur_predictor_kernel", "predictor_hidden", "audio_num_mel_bins", "ffn_padding_same",
              "ffn_act_gelu", "dur_loss_mse", "rel_pos", "use_pos_embed", "encoder_fft", "decoder_fft", "use_pitch_embed",
              "use_energy_embed", "use_spk_id", "use_spk_embed", "use_bert"]
NEW_FIELDS = ["plain", "num_spk", "use_split_spk_id", "predictor_layers", "predictor_kernel"]
NEW_ENTRIES = ("maa_fs2_encode_plain", "maa_fs2_speaker", "maa_fs2_add_speaker", "maa_fs2_finish", "maa_fs2_pitch_forward_from")
# sha256 of make_fs2_state_dict(C.FASTSPEECH2_MIDI, seed=17), as tests/test_fs2_pitch_host.py pins it
FS2_SEED17_HASH = "158bb7716b2fe9a67db52d38405db15b83fdec214f2c431467d4d2bda67e2f1a"
GATE = 2e-4
ENERGY = dict(C.FASTSPEECH2, use_energy_embed=True)
SPLIT = dict(ENERGY, use_spk_id=True, use_split_spk_id=True, num_spk=7)


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)


def _t(g, k):
    return torch.from_numpy(g[k]) if k in g else None


def test_config_structure_matches_header_old_fields_first():
    from audiogpt_amd import _lib
    body = re.search(r"typedef struct maa_fs2_config \{(.*?)\} maa_fs2_config;", _header(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            assert ctype == "int"
            fields += [n.strip() for n in names.split(",")]
    assert fields == [n for n, _ in _lib.maa_fs2_config._fields_]
    assert all(t is ctypes.c_int for _, t in _lib.maa_fs2_config._fields_)
    assert fields == OLD_FIELDS + NEW_FIELDS
    assert ctypes.sizeof(_lib.maa_fs2_config) == 4 * len(fields)


def test_new_entries_are_declared_and_bound(lib):
    from audiogpt_amd import _lib
    src = _header()
    for name in NEW_ENTRIES:
        assert name in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")), name


def test_configurations():
    from audiogpt_amd import backend
    c = C.FASTSPEECH2
    assert (c["enc_layers"], c["dec_layers"], c["num_heads"], c["enc_ffn_kernel_size"], c["dec_ffn_kernel_size"]) == (4, 4, 2, 9, 9)
    assert (c["dur_predictor_layers"], c["dur_predictor_kernel"], c["predictor_layers"], c["predictor_kernel"]) == (2, 3, 2, 5)
    assert c["use_pitch_embed"] is True and c["pitch_type"] == "frame" and c["use_uv"] is True and c["pitch_norm"] == "standard"
    assert c["rel_pos"] is False and c["use_energy_embed"] is False and c["use_spk_id"] is False
    lt = C.FASTSPEECH2_LIBRITTS
    assert lt["use_spk_id"] is True and lt["num_spk"] == 2320 and {k: v for k, v in lt.items() if k not in ("use_spk_id", "num_spk")} == \
        {k: v for k, v in c.items() if k not in ("use_spk_id", "num_spk")}
    s = backend.fs2_plain_config(dict(SPLIT, use_pitch_embed=False, predictor_hidden=384))
    assert (s.plain, s.rel_pos, s.use_pos_embed, s.use_energy_embed, s.use_spk_id, s.use_spk_embed, s.use_split_spk_id) == (1, 0, 1, 1, 1, 0, 1)
    assert (s.num_spk, s.predictor_layers, s.predictor_kernel, s.predictor_hidden, s.use_pitch_embed, s.use_bert) == (7, 2, 5, 384, 0, 0)
    r = backend.fs2_plain_config(dict(c, use_pitch_embed=False, rel_pos=True, use_spk_embed=True))
    assert (r.plain, r.rel_pos, r.use_spk_id, r.use_spk_embed, r.num_spk) == (1, 1, 0, 1, 0)
    # the MIDI handle's configuration is today's: the appended fields stay zero
    m = backend.fs2_config(C.FASTSPEECH2_MIDI)
    assert [getattr(m, k) for k in NEW_FIELDS] == [0] * 5


PLAIN_REFUSALS = [(dict(use_bert=True), "use_bert"), (dict(use_pos_embed=False), "use_pos_embed"), (dict(ffn_padding="LEFT"), "SAME"),
                  (dict(ffn_act="relu"), "gelu"), (dict(dur_loss="huber"), "mse"), (dict(encoder_type="conformer"), "fft"),
                  (dict(decoder_type="conv"), "fft"), (dict(num_heads=4), "128"), (dict(use_spk_id=True, use_spk_embed=True), "alternatives"),
                  (dict(use_split_spk_id=True), "use_split_spk_id"), (dict(use_spk_id=True, num_spk=0), "num_spk"),
                  (dict(pitch_type="ph"), "pitch_type 'ph'"), (dict(pitch_type="cwt"), "no oracle"), (dict(pitch_ar=True), "pitch_ar"),
                  (dict(pitch_norm="minmax"), "pitch_norm")]


@pytest.mark.parametrize("change,reason", PLAIN_REFUSALS)
def test_unsupported_configuration_is_refused_with_the_reason_before_a_context(change, reason, monkeypatch):
    from audiogpt_amd import _lib, diffsinger
    monkeypatch.setattr(diffsinger, "Context", lambda *a, **k: pytest.fail("a context was made before the configuration was refused"))
    with pytest.raises(_lib.MaaError, match=reason):
        diffsinger.FastSpeech2(dict(C.FASTSPEECH2, **change))


def test_backend_config_refuses_the_pitch_branch_and_the_midi_refusals_stay():
    from audiogpt_amd import _lib, backend
    with pytest.raises(_lib.MaaError, match="FS2Pitch beside it"):
        backend.fs2_plain_config(C.FASTSPEECH2)
    for change, reason in ((dict(rel_pos=False), "rel_pos"), (dict(use_energy_embed=True), "use_energy_embed"),
                           (dict(use_spk_id=True), "use_spk_id"), (dict(use_spk_embed=True), "use_spk_embed")):
        with pytest.raises(_lib.MaaError, match=reason):
            backend.fs2_config(dict(C.FASTSPEECH2_MIDI, **change))
    for k in ("use_energy_embed", "use_spk_id", "use_spk_embed"):
        with pytest.raises(_lib.MaaError, match=k):
            backend.fs2_pitch_config(dict(C.FASTSPEECH2_MIDI_CASCADE, **{k: True}))


LIB_REFUSALS = [("use_pitch_embed", 1, b"maa_fs2_pitch"), ("use_bert", 1, b"use_bert"), ("num_heads", 4, b"128"), ("hidden_size", 192, b"128"),
                ("use_pos_embed", 0, b"use_pos_embed"), ("ffn_padding_same", 0, b"SAME"), ("ffn_act_gelu", 0, b"gelu"),
                ("dur_loss_mse", 0, b"mse"), ("encoder_fft", 0, b"fft"), ("predictor_kernel", 4, b"odd"), ("num_spk", 0, b"num_spk")]


@pytest.mark.parametrize("field,value,reason", LIB_REFUSALS)
def test_library_refuses_a_plain_config_with_a_null_context(lib, field, value, reason):
    from audiogpt_amd import backend
    cfg = backend.fs2_plain_config(dict(SPLIT, use_pitch_embed=False))
    setattr(cfg, field, value)
    h = ctypes.c_void_p()
    assert lib.maa_fs2_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0
    assert reason in lib.maa_last_error() and b"null context" not in lib.maa_last_error(), lib.maa_last_error()


def test_library_accepts_the_plain_flags_up_to_the_context_and_keeps_the_midi_refusals(lib):
    from audiogpt_amd import backend
    h = ctypes.c_void_p()
    for cfg in (dict(SPLIT, use_pitch_embed=False), dict(C.FASTSPEECH2, use_pitch_embed=False, rel_pos=True, use_spk_embed=True)):
        c = backend.fs2_plain_config(cfg)
        assert lib.maa_fs2_create(None, ctypes.byref(c), None, 0, ctypes.byref(h)) < 0
        assert b"null context" in lib.maa_last_error(), lib.maa_last_error()
    for field, value, reason in (("rel_pos", 0, b"rel_pos"), ("use_energy_embed", 1, b"use_energy_embed"), ("use_spk_id", 1, b"use_spk_id"),
                                 ("use_spk_embed", 1, b"use_spk_embed"), ("use_pitch_embed", 1, b"use_pitch_embed")):
        c = backend.fs2_config(C.FASTSPEECH2_MIDI)
        setattr(c, field, value)
        assert lib.maa_fs2_create(None, ctypes.byref(c), None, 0, ctypes.byref(h)) < 0
        assert reason in lib.maa_last_error() and b"FastSpeech2MIDI" in lib.maa_last_error(), lib.maa_last_error()


def test_bad_sizes_fail_before_the_context_is_touched(lib):
    """Non-null garbage pointers: the size check answers first, nothing is dereferenced."""
    p, q, r = ctypes.c_void_p(64), ctypes.c_void_p(128), ctypes.c_void_p(192)
    for B, T in ((0, 4), (4, 0), (1 << 10, 1 << 10)):
        assert lib.maa_fs2_encode_plain(p, p, p, p, B, T, p, p, p, p) < 0
        assert b"B, T" in lib.maa_last_error()
        assert lib.maa_fs2_add_speaker(p, p, p, p, p, B, T, p) < 0
        assert b"B, T_mel" in lib.maa_last_error()
        assert lib.maa_fs2_finish(p, p, p, q, p, p, p, B, T, r, p, p) < 0
        assert b"B, T_mel" in lib.maa_last_error()
        assert lib.maa_fs2_pitch_forward_from(p, p, p, q, p, p, p, B, T, r, p, p, p) < 0
        assert b"B, T_mel" in lib.maa_last_error()
    for B in (0, 1 << 20):
        assert lib.maa_fs2_speaker(p, p, p, p, B, p) < 0
        assert b"arguments: B" in lib.maa_last_error()
    assert lib.maa_fs2_speaker(p, p, None, None, 1, p) < 0 and b"neither" in lib.maa_last_error()
    assert lib.maa_fs2_finish(p, p, p, q, p, p, p, 1, 1, q, p, p) < 0 and b"alias" in lib.maa_last_error()
    assert lib.maa_fs2_pitch_forward_from(p, p, p, q, p, p, p, 1, 1, q, p, p, p) < 0 and b"alias" in lib.maa_last_error()


def test_state_dict_keys_are_the_references_in_order():
    for name in sorted({n for n, _ in R.CASES}):
        cfg, sd, g = R.load_case(name)
        assert list(sd.keys()) == g["keys"], name
    cfg, sd, g = R.load_case("fs2_plain_energy_spk_b2_t33")
    assert len(sd) == 130 and "encoder.embed_positions._float_tensor" in sd
    keys = list(sd)
    assert keys.index("spk_embed_proj.weight") < keys.index("spk_embed_f0.weight") < keys.index("spk_embed_dur.weight") \
        < keys.index("dur_predictor.conv.0.1.weight") < keys.index("pitch_embed.weight") < keys.index("energy_embed.weight")
    H = cfg["hidden_size"]
    assert tuple(sd["energy_embed.weight"].shape) == (256, H) and tuple(sd["energy_predictor.linear.weight"].shape) == (1, H)
    assert tuple(sd["spk_embed_dur.weight"].shape) == (8, H) and float(sd["energy_predictor.pos_embed_alpha"]) != 1.0
    assert sd["encoder.embed_tokens.weight"] is sd["encoder_embed_tokens.weight"]
    # the shared tensors do not depend on the optional branches
    plain = WT.make_fs2_plain_state_dict(dict(C.FASTSPEECH2, use_pitch_embed=False), seed=R.SEED)
    full = WT.make_fs2_plain_state_dict(SPLIT, seed=R.SEED)
    assert all(torch.equal(plain[k], full[k]) for k in plain)
    emb = WT.make_fs2_plain_state_dict(dict(C.FASTSPEECH2, use_spk_embed=True), seed=R.SEED)
    assert tuple(emb["spk_embed_proj.weight"].shape) == (H, 256) and tuple(emb["spk_embed_proj.bias"].shape) == (H,)


def test_the_midi_state_dict_is_unchanged():
    """Against the pinned hash and against the tensors the existing goldens' loaders produce."""
    assert P.state_dict_hash(WT.make_fs2_state_dict(C.FASTSPEECH2_MIDI, seed=17)) == FS2_SEED17_HASH
    from tests import fs2_ref
    for name in ("fs2_b2_t33", "fs2_ph384_b2_t9"):
        cfg, sd, _ = fs2_ref.load_case(name)
        again = WT.make_fs2_state_dict(cfg, seed=17)
        assert list(again) == list(sd)
        assert all(torch.equal(again[k], sd[k]) for k in sd if k != "dur_predictor.linear.bias"), name
    cfg, sd, _ = P.load_case("fs2_pitch_b2_t33")
    again = WT.make_fs2_state_dict(cfg, seed=17)
    moved = ("dur_predictor.linear.bias", "pitch_predictor.linear.weight", "pitch_predictor.linear.bias")
    assert list(again) == list(sd) and all(torch.equal(again[k], sd[k]) for k in sd if k not in moved)


def test_counted_positions():
    tok = torch.tensor([[3, 4, 5, 6, 0, 7, 8], [1, 0, 0, 2, 0, 0, 0]])
    assert R.positions(tok).tolist() == [[1, 2, 3, 4, 0, 5, 6], [1, 0, 0, 2, 0, 0, 0]]
    _, _, g = R.load_case("fs2_plain_b2_t33")
    tok = _t(g, "txt_tokens")
    pos = R.positions(tok)
    assert int(tok[0, 11]) == 0 and int(pos[0, 11]) == 0 and int(pos[0, 12]) == 12          # indexed positions would say 13
    assert bool((tok[1, 20:] == 0).all()) and int(pos[1].max()) == 20


@pytest.mark.parametrize("name,prefix", [c for c in R.CASES if c[0] != "fs2_plain_energy_spk_b2_t33"])
def test_embed_restatement_matches_reference(name, prefix):
    """To 4 x the reference's own fp32 - fp64 difference on the live rows (the reference masks after the embedding)."""
    cfg, sd, g = R.load_case(name, prefix)
    tok = _t(g, "txt_tokens")
    x = R.embed(cfg, tok, sd["encoder.embed_tokens.weight"])
    live = tok != 0
    err, floor = float((x - _t(g, "embed"))[live].abs().max()), float(g["floor_embed"])
    print("%s%s: embed %.2e (floor %.2e)" % (name, prefix, err, floor))
    assert floor > 0 and err <= 4 * floor
    assert bool((x[~live] == 0).all())
    if not cfg["rel_pos"] and bool((~live[:, :-1]).any()):
        # a port that indexed the positions, or scaled twice, is far outside the floor
        H = cfg["hidden_size"]
        indexed = H ** 0.5 * sd["encoder.embed_tokens.weight"][tok] + R.sinusoid_table(tok.shape[1] + 1, H)[torch.arange(1, tok.shape[1] + 1)][None]
        assert float((indexed - _t(g, "embed"))[live].abs().max()) > 1e-2 or name != "fs2_plain_b2_t33"


@pytest.mark.parametrize("name,prefix", [c for c in R.CASES if "energy_pred" in R.load_case(*c)[2]])
def test_energy_tail_restatement_matches_reference(name, prefix):
    """From the golden's energy_pred and the decoder_inp so far: bins exactly off the flagged frames, decoder_inp to 4 x the
    reference's own fp32 - fp64 difference on the rows whose bin agrees."""
    cfg, sd, g = R.load_case(name, prefix)
    m2p, live = _t(g, "mel2ph"), _t(g, "mel2ph") > 0
    acc = R.origin(g) + sd["pitch_embed.weight"][_t(g, "coarse")]
    spk = _t(g, "spk")[0] if "spk" in g else None
    e_in = _t(g, "energy_in")
    before = None if e_in is None else e_in.clone()
    bins, dec = R.energy_tail(acc, _t(g, "energy_pred"), m2p, sd["energy_embed.weight"], spk=spk, energy=e_in)
    assert before is None or torch.equal(e_in, before)
    fl = _t(g, "energy_flagged")
    assert torch.equal(bins[~fl], _t(g, "energy_bin")[~fl]) and int((bins - _t(g, "energy_bin")).abs().max()) <= 1
    rows = bins == _t(g, "energy_bin")
    err, floor = float((dec - _t(g, "decoder_inp"))[rows].abs().max()), float(g["floor_decoder_inp"])
    print("%s%s: decoder_inp %.2e (floor %.2e), energy flagged %d" % (name, prefix, err, floor, int(fl.sum())))
    assert floor > 0 and err <= 4 * floor
    assert bool((dec[~live] == 0).all())
    if e_in is not None:
        assert not bool(fl.any()) and torch.equal(bins, _t(g, "energy_bin"))
    assert R.energy_bin(torch.tensor([-0.5, 0.0, 1.0 / 64, 3.99, 4.0, 7.0])).tolist() == [0, 0, 1, 255, 255, 255]


def test_golden_cases_are_what_the_tests_need():
    for name, prefix in R.CASES:
        cfg, _, g = R.load_case(name, prefix)
        live = g["mel2ph"] > 0
        assert g["flagged"].sum() <= 0.3 * live.sum() and not g["flagged"][~live].any(), name
        if "uv_in" not in g:
            assert (np.abs(g["pitch_pred"][..., 1][live]) > GATE * np.abs(g["pitch_pred"]).max()).all(), name
        if cfg["use_energy_embed"]:
            assert g["energy_flagged"].sum() <= 0.3 * live.sum() and not g["energy_flagged"][~live].any(), name
            assert g["energy_pred"].min() >= 0 and g["energy_bin"].min() >= 0 and g["energy_bin"].max() <= 255
    cfg, _, g = R.load_case("fs2_plain_b2_t33")
    assert {k: cfg[k] for k in C.FASTSPEECH2} == C.FASTSPEECH2
    assert g["txt_tokens"][0, 11] == 0 and (g["txt_tokens"][0, 12:] > 0).all() and (g["txt_tokens"][1, 20:] == 0).all()
    tot = (g["mel2ph"] > 0).sum(-1)
    assert g["mel2ph"].shape[1] > 128 and int(tot.max() - tot.min()) >= 64 and "dur_choice" in g
    cfg, _, g = R.load_case("fs2_plain_energy_spk_b2_t33")
    live = g["mel2ph"] > 0
    assert cfg["use_energy_embed"] and cfg["use_spk_id"] and cfg["use_split_spk_id"] and cfg["num_spk"] == 7
    ids = g["spk_ids"]
    assert ids.shape == (3, 2) and all(len(set(ids[:, b].tolist())) == 3 for b in range(2)) and int((ids == 0).sum()) == 1
    assert len(np.unique(g["energy_bin"][live])) >= 20 and (g["energy_bin"][live] == 255).any() and g["energy_flagged"].any()
    assert abs(float(g["energy_pred"].min()) - 0.05) < 1e-3 and abs(float(g["energy_pred"][live].max()) - 4.3) < 1e-3
    cfg, _, g = R.load_case("fs2_plain_given")
    assert cfg["use_spk_embed"] and cfg["pitch_norm"] == "log" and g["spk_vec"].shape == (2, 256) and "dur_choice" not in g
    assert g["mel2ph_in"].shape == (2, 70) and (g["mel2ph_in"] > 0).sum(-1).tolist() == [66, 40]
    assert g["energy_bin"][0, :5].tolist() == [0, 1, 254, 255, 255] and float(g["energy_in"][0, 4]) > 4.0
    assert not g["flagged"].any() and not g["energy_flagged"].any() and all(k in g for k in ("f0_in", "uv_in", "energy_in"))
    for p in ("t1.", "t4."):
        cfg, _, s = R.load_case("fs2_plain_short", p)
        assert s["mel2ph"].shape[1] < 9 and s["txt_tokens"].shape == (1, int(p[1])) and cfg["use_energy_embed"]
    cfg, _, g = R.load_case("fs2_plain_relpos_b2_t9")
    assert cfg["rel_pos"] is True and cfg["enc_layers"] == cfg["dec_layers"] == 1 and (g["txt_tokens"][1, 6:] == 0).all()
    cfg, _, g = R.load_case("fs2_plain_ph384_b2_t9")
    assert cfg["predictor_hidden"] == 384 and cfg["use_energy_embed"]
    for name in sorted({n for n, _ in R.CASES}):
        assert os.path.getsize(os.path.join(R.GOLDEN, name + ".npz")) <= 402647          # the largest fs2_pitch_* file


class _NoDevice:
    device = "cpu"


def _hostonly(cfg):
    """A diffsinger.FastSpeech2 without its handles: the host checks run before any device call."""
    from audiogpt_amd import diffsinger
    m = object.__new__(diffsinger.FastSpeech2)
    m.cfg = dict(cfg)
    m.use_pitch, m.use_energy = bool(cfg.get("use_pitch_embed")), bool(cfg.get("use_energy_embed"))
    m.spk_mode = "id" if cfg.get("use_spk_id") else "embed" if cfg.get("use_spk_embed") else None
    m.device = "cpu"

    class Net:
        def __getattr__(self, name):
            raise _Reached(name)
    m.net = Net()
    return m


class _Reached(Exception):
    pass


def test_host_checks_of_ids_tokens_and_energy():
    tok = torch.tensor([[1, 2, 3, 0]])
    m = _hostonly(SPLIT)
    with pytest.raises(ValueError, match="vocab_size"):
        m(torch.tensor([[1, 64]]), spk_embed=torch.tensor([1]))
    with pytest.raises(ValueError, match="no live token"):
        m(torch.tensor([[0, 0]]), spk_embed=torch.tensor([1]))
    with pytest.raises(ValueError, match="needs spk_embed"):
        m(tok)
    for bad in (torch.tensor([8]), torch.tensor([-1])):
        with pytest.raises(ValueError, match=r"spk_embed outside \[0, num_spk = 7\]"):
            m(tok, spk_embed=bad)
    with pytest.raises(ValueError, match="spk_embed_f0_id outside"):
        m(tok, spk_embed=torch.tensor([7]), spk_embed_f0_id=torch.tensor([9]))
    with pytest.raises(ValueError, match="integer ids"):
        m(tok, spk_embed=torch.tensor([1.0]))
    with pytest.raises(ValueError, match="mel2ph outside"):
        m(tok, spk_embed=torch.tensor([7]), mel2ph=torch.tensor([[1, 5]]))
    with pytest.raises(_Reached, match="speaker"):          # ids 0 and num_spk are rows of the table
        m(tok, spk_embed=torch.tensor([7]), spk_embed_dur_id=torch.tensor([0]))
    ids = m._speaker_ids(torch.tensor([3]), None, torch.tensor([5]), 1)
    assert ids.tolist() == [[3], [3], [5]]
    e = _hostonly(dict(ENERGY, use_spk_embed=True))
    with pytest.raises(ValueError, match=r"spk_embed \[B = 1, 256\]"):
        e(tok, spk_embed=torch.zeros(1, 128))
    with pytest.raises(ValueError, match="infer=True"):
        e(tok, infer=False)
    for bad in (torch.tensor([[0.5, -0.01]]), torch.tensor([[float("nan"), 1.0]])):
        with pytest.raises(ValueError, match="energy below 0"):
            e(tok, spk_embed=torch.zeros(1, 256), energy=bad)
    with pytest.raises(_Reached, match="speaker"):
        e(tok, spk_embed=torch.zeros(1, 256), energy=torch.tensor([[0.0, 4.5]]))
    with pytest.raises(_Reached):          # a model without the energy branch does not read the argument, as the reference
        _hostonly(C.FASTSPEECH2)(tok, energy=torch.tensor([[-1.0]]))


def test_new_kernels_do_not_spill(tmp_path):
    """vgpr_spill_count and the private segment of the plain model's kernels in the cross-compiled gfx950 assembly's metadata (read
    as tests/test_fs2_pitch_host.py::test_new_kernels_do_not_spill reads it)."""
    from audiogpt_amd.build import FLAGS
    csrc = os.path.join(ROOT, "audiogpt_amd", "csrc")
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path / "fs2.s")
    cmd = [hipcc] + [f for f in FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                                                          os.path.join(csrc, "fs2.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", open(out).read()):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    wanted = ("fs2_token_positions_kernel", "fs2_embed_plain_kernel", "fs2_add_speaker_kernel", "fs2_speaker_gather_kernel",
              "fs2_energy_tail_kernelILi1E", "fs2_energy_tail_kernelILi2E", "fs2_energy_tail_kernelILi4E")
    new = {k: v for k, v in meta.items() if any(w in k for w in wanted)}
    assert len(new) == len(wanted), sorted(new)
    for name, (private, vg, spill) in new.items():
        print(name, "vgprs", vg)
        assert spill == 0 and private == 0, (name, private, spill)
        assert vg <= 128, (name, vg)          # row kernels: four waves per SIMD
