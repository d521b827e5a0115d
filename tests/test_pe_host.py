"""CPU checks of the PitchExtractor work: the host restatement (tests/pe_ref.py) against the reference's own outputs
(tests/golden/pe_*.npz, written by tests/golden/make_golden_pe.py), the state-dict key layout, make_positions, the C ABI
entries, the refusal of a padding mode that is not built, and the register metadata of csrc/pitch.hip's kernels."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import pe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audiogpt_amd", "csrc")
ENTRIES = ("maa_pitch_extractor_create", "maa_pitch_extractor_destroy", "maa_pitch_extractor_forward")


@pytest.mark.parametrize("name,prefix", R.CASES)
def test_restatement_matches_reference(name, prefix):
    """Gate: 10 x the reference's own fp32 - fp64 difference of the case (recorded by the generator), relative to max|reference|."""
    cfg, sd, g = R.load_case(name, prefix)
    mel = torch.from_numpy(g["mel"])
    with torch.no_grad():
        hidden, pp, f0 = R.forward(sd, cfg, mel)
        hidden64, pp64, _ = R.forward(sd, cfg, mel.double())
    for what, got, got64, ref, floor in (("mel_hidden", hidden, hidden64, g["mel_hidden"], float(g["floor_mel_hidden"])),
                                         ("pitch_pred", pp, pp64, g["pitch_pred"], float(g["floor_pitch_pred"]))):
        ref = torch.from_numpy(ref)
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        err64 = float((got64 - ref.double()).abs().max())
        print("%s%s %s: fp32 restatement %.2e, fp64 restatement %.2e, recorded floor %.2e, max|ref| %.2f" % (name, prefix, what, err, err64, floor, scale))
        assert floor > 0
        assert err / scale <= 10 * floor / scale, (what, err, floor)
        assert err64 / scale <= 10 * floor / scale, (what, err64, floor)
    # f0: zero / non-zero as the reference (the generator keeps every voicing logit clear of 0), padding exactly 0
    ref_f0 = torch.from_numpy(g["f0_denorm_pred"])
    assert torch.equal(f0 == 0, ref_f0 == 0)
    assert bool((f0[mel.abs().sum(-1) == 0] == 0).all())
    voiced = ref_f0 != 0
    # d(2 ** x) = ln 2 * 2 ** x * dx, d(x * std + mean) = std * dx, with dx within the pitch_pred gate; plus the two results' own
    # rounding (<= 2 ulp each of |f0|: pow is not correctly rounded)
    dx, ulp = 10 * float(g["floor_pitch_pred"]), 4 * 2.0 ** -23 * ref_f0[voiced].abs()
    bound = (0.6931472 * dx * ref_f0[voiced].abs() if cfg["pitch_norm"] == "log" else dx * cfg["f0_std"]) + ulp
    assert bool(((f0 - ref_f0)[voiced].abs() <= bound).all())


def test_state_dict_keys_match_reference():
    for name in sorted({n for n, _ in R.CASES}):
        cfg, sd, g = R.load_case(name)
        assert sorted(sd.keys()) == sorted(g["keys"]), name
    assert len(WT.make_pe_state_dict(C.PITCH_EXTRACTOR)) == 59
    sd = WT.make_pe_state_dict(C.PITCH_EXTRACTOR)
    for i in range(3):
        p = "mel_prenet.layers.%d.2." % i
        assert float(sd[p + "running_mean"].std()) > 0.2 and 0.5 <= float(sd[p + "running_var"].min()) and float(sd[p + "running_var"].max()) <= 1.5
        assert float((sd[p + "weight"] - 1).abs().max()) > 0.05 and float(sd[p + "bias"].abs().max()) > 0.05
    assert float(sd["pitch_predictor.pos_embed_alpha"]) != 1.0


def test_make_positions_skips_zeros():
    ch0 = torch.tensor([[0.0, 0.0, 1.5, -2.0, 0.0, 3.0, -0.0, 4.0, 0.0, 0.0],
                        [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0]])
    pos = R.make_positions(ch0)
    assert pos.tolist() == [[0, 0, 1, 2, 0, 3, 0, 4, 0, 0], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]]
    tab = R.sinusoid_table(12, 8)
    assert bool((tab[0] == 0).all()) and abs(float(tab[1, 0]) - 0.8414710) < 1e-6 and float(tab[3, 4]) == pytest.approx(-0.9899925, abs=1e-6)


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_abi_entries_are_declared_bound_and_reject_null(lib):
    from audiogpt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")), name
    h = ctypes.c_void_p()
    assert lib.maa_pitch_extractor_create(None, None, None, 0, ctypes.byref(h)) < 0
    assert b"null" in lib.maa_last_error()
    cfg = _backend_cfg(C.PITCH_EXTRACTOR)
    assert lib.maa_pitch_extractor_create(None, ctypes.byref(cfg), None, 0, None) < 0
    assert b"null" in lib.maa_last_error()
    assert lib.maa_pitch_extractor_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0      # no context
    assert b"null" in lib.maa_last_error()
    assert lib.maa_pitch_extractor_forward(None, None, None, 1, 1, None, None, None) < 0
    assert len(lib.maa_last_error()) > 0
    assert lib.maa_pitch_extractor_destroy(None) == 0


def _backend_cfg(cfg):
    from audiogpt_amd import backend
    return backend.pe_config(cfg)


def test_non_same_padding_is_refused(lib):
    from audiogpt_amd import _lib
    with pytest.raises(_lib.MaaError, match="SAME"):
        _backend_cfg(dict(C.PITCH_EXTRACTOR, ffn_padding="LEFT"))
    # the library refuses it too, with the reason, before it touches a device
    cfg = _backend_cfg(C.PITCH_EXTRACTOR)
    cfg.ffn_padding_same = 0
    h = ctypes.c_void_p()
    assert lib.maa_pitch_extractor_create(None, ctypes.byref(cfg), None, 0, ctypes.byref(h)) < 0
    assert b"SAME" in lib.maa_last_error()
    # and the reference-surface class before it makes a context
    from audiogpt_amd.diffsinger import PitchExtractor
    with pytest.raises(_lib.MaaError, match="SAME"):
        PitchExtractor(dict(C.PITCH_EXTRACTOR, ffn_padding="LEFT"))


def test_pitch_kernels_do_not_spill(tmp_path):
    """vgpr_spill_count of every kernel of pitch.hip in the cross-compiled gfx950 assembly's metadata (read as
    tests/test_isa_guards.py::test_register_budgets reads it)."""
    from audiogpt_amd.build import FLAGS
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path / "pitch.s")
    cmd = [hipcc] + [f for f in FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                                          os.path.join(CSRC, "pitch.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    meta = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    names = " ".join(meta)
    for k in ("pe_frame_mask_kernel", "pe_affine_mask_kernel", "pe_gn_stats_kernel", "pe_gn_relu_res_kernel", "pe_positions_kernel",
              "pe_pos_add_kernel", "pe_head_kernel"):
        assert k in names, k
    assert len(meta) >= 9          # three widths of the head kernel
    for name, (vg, spill) in meta.items():
        assert spill == 0, (name, spill)
        assert vg <= 128, (name, vg)          # four waves per SIMD: these kernels hide latency by occupancy
