"""CPU checks of the Glow post-net work: the host restatement (tests/glow_ref.py) against the reference's own outputs
(tests/golden/glow_*.npz and postglow_*.npz, written by tests/golden/make_golden_glow.py), the seeded state-dict factory's key
layout, the refusals of the Python classes and of the library (by message, with no device), the C ABI entries and the
configuration structure against the header, the zero-config rule, and the host draw of PostGlow."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from tests import glow_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = {"maa_glow_create": 5, "maa_glow_destroy": 1, "maa_glow_reverse": 10}
GLOW_CASES, load_case = R.CASES, R.load_case


def test_every_golden_is_listed():
    found = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "glow_*.npz")))
    assert found == sorted(GLOW_CASES)
    assert os.path.exists(os.path.join(GOLDEN, "postglow_gs_t40.npz"))


@pytest.mark.parametrize("name", GLOW_CASES)
def test_restatement_matches_reference(name):
    """x, logdet and every entry of hs within 8 x the reference's own fp32 - fp64 difference plus 1e-6 of the maximum."""
    cfg, sd, g = load_case(name)
    t = lambda k: torch.from_numpy(g[k]) if k in g.files else None          # noqa: E731
    with torch.no_grad():
        x, logdet, hs = R.glow_reverse(sd, cfg, t("z"), t("mask"), t("g"), return_hiddens=True)
    T = g["z"].shape[2]
    assert x.shape == (g["z"].shape[0], cfg["in_channels"], 2 * (T // 2)) and len(hs) == 3 * cfg["n_blocks"]

    def close(what, got, ref, floor):
        ref = torch.from_numpy(np.asarray(ref))
        err, bound = float((got - ref).abs().max()), 8 * float(floor) + 1e-6 * float(ref.abs().max())
        print("%s %s: restatement %.2e, bound %.2e, max|ref| %.3g" % (name, what, err, bound, float(ref.abs().max())))
        assert err <= bound, (what, err, bound)

    close("x", x, g["x"], g["floor_x"])
    close("logdet", logdet, g["logdet"], g["floor_logdet"])
    for i, h in enumerate(hs):
        close("hs[%d]" % i, h, g["hs"][i], g["floor_hs"][i])
    # exact zeros on every masked frame, pairs cut by the mask included
    live = torch.from_numpy(g["mask"])[:, 0, 1::2].repeat_interleave(2, dim=1)
    assert bool((x.transpose(1, 2)[live == 0] == 0).all())


def test_restatement_of_run_post_glow_matches_reference():
    cfg, sd, g = load_case("postglow_gs_t40")
    t = lambda k: torch.from_numpy(g[k])          # noqa: E731
    torch.manual_seed(int(g["draw_seed"]))
    with torch.no_grad():
        x = R.post_glow_infer(sd, cfg, t("mel_out"), t("decoder_inp"), t("spk_embed"), t("emo_embed"), t("ref_prosody"))
        xz = R.post_glow_infer(sd, cfg, t("mel_out"), t("decoder_inp"), t("spk_embed"), t("emo_embed"), t("ref_prosody"), z=t("z"))
    ref = t("x")
    bound = 8 * float(g["floor_x"]) + 1e-6 * float(ref.abs().max())
    assert float((x - ref).abs().max()) <= bound and float((xz - ref).abs().max()) <= bound


def test_seeded_factory_has_the_reference_key_layout():
    for name in GLOW_CASES + ("postglow_gs_t40",):
        cfg, sd, g = load_case(name)
        assert sorted(sd) == list(g["keys"]), name
        assert [",".join(str(s) for s in sd[k].shape) for k in sorted(sd)] == list(g["key_shapes"]), name
    gs = WT.make_glow_state_dict(C.GENERSPEECH_POST_GLOW)
    assert len(gs) == 280 and len(WT.make_glow_state_dict(C.PORTASPEECH_POST_GLOW)) == 420
    assert abs(sum(v.numel() for v in gs.values()) - 16.9e6) < 0.1e6
    assert C.GENERSPEECH_POST_GLOW["gin_channels"] == 1104 and C.PORTASPEECH_POST_GLOW["gin_channels"] == 272
    assert C.GENERSPEECH_POST_GLOW["noise_scale"] == C.PORTASPEECH_POST_GLOW["noise_scale"] == 0.8
    for b in range(8):
        pa, pi, pc = "flows.%d." % (3 * b), "flows.%d." % (3 * b + 1), "flows.%d." % (3 * b + 2)
        # what the reference initialises to nothing is drawn
        for k in (pc + "end.weight", pc + "end.bias", pa + "logs", pa + "bias"):
            assert float(gs[k].abs().max()) > 0.01, k
        p, sign = gs[pi + "p"], gs[pi + "sign_s"]
        assert not torch.equal(p, torch.eye(4)) and bool((p.sum(0) == 1).all()) and bool((p.sum(1) == 1).all())
        assert float(sign.min()) == -1.0 and float(sign.max()) == 1.0
        assert torch.equal(gs[pi + "l_mask"], torch.tril(torch.ones(4, 4), -1)) and torch.equal(gs[pi + "eye"], torch.eye(4))
        # share_wn_layers 4: a group's members repeat the lead's tensors; the groups differ
        lead = "flows.%d." % (3 * (b - b % 4) + 2)
        assert torch.equal(gs[pc + "wn.in_layers.1.weight_v"], gs[lead + "wn.in_layers.1.weight_v"])
        assert b % 4 == 0 or not torch.equal(gs[pc + "wn.cond_layer.weight_v"], gs[lead + "wn.cond_layer.weight_v"])
    assert not torch.equal(gs["flows.2.wn.in_layers.0.weight_v"], gs["flows.14.wn.in_layers.0.weight_v"])


def test_python_refusals_by_message():
    """Before a device is touched: there is none here, so a refusal that came later would be the missing GPU's."""
    from audiogpt_amd import _lib, backend
    from audiogpt_amd.generspeech import Glow, check_shared_wn
    GS = C.GENERSPEECH_POST_GLOW
    for over, message in ((dict(inv_conv_type="invconv"), "inv_conv_type"), (dict(n_sqz=1), "n_sqz"), (dict(n_split=2), "n_split"),
                          (dict(kernel_size=4), "kernel_size"), (dict(hidden_channels=127), "hidden_channels"),
                          (dict(in_channels=78), "in_channels % 4 != 0")):
        with pytest.raises(_lib.MaaError, match=message):
            backend.glow_config(dict(GS, **over))
        with pytest.raises(_lib.MaaError, match=message):
            Glow(dict(GS, **over))
    backend.glow_config(dict(GS, p_dropout=0.5))          # ignored (eval)
    # a state dict whose group members differ
    small = dict(GS, in_channels=8, hidden_channels=8, gin_channels=4, n_blocks=2, share_wn_layers=2)
    sd = WT.make_glow_state_dict(small)
    check_shared_wn(small, sd)
    sd["flows.5.wn.res_skip_layers.0.weight_v"] = sd["flows.5.wn.res_skip_layers.0.weight_v"] + 1.0
    with pytest.raises(_lib.MaaError, match="share_wn_layers = 2 but flows.5.wn.res_skip_layers.0.weight_v differs"):
        check_shared_wn(small, sd)
    with pytest.raises(_lib.MaaError, match="share_wn_layers"):
        Glow(small, state_dict=sd)
    # the training direction and a single frame: refused by the class before the handle is used
    glow = Glow.__new__(Glow)
    glow.cfg = dict(GS)
    with pytest.raises(_lib.MaaError, match="reverse=False"):
        glow(torch.zeros(1, 80, 8), None, g=None)
    with pytest.raises(_lib.MaaError, match="T < 2"):
        glow(torch.zeros(1, 80, 1), None, g=None, reverse=True)


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_abi_entries_are_declared_exported_and_bound(lib):
    from audiogpt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    for name, n in ENTRIES.items():
        assert name in _lib.EXPORTS and hasattr(lib, name)
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert decl, name
        assert len(getattr(lib, name).argtypes) == len(decl.group(1).split(",")) == n, name
    body = re.search(r"typedef struct \{([^}]*)\} maa_glow_config;", src).group(1)
    fields = [f.strip() for f in re.sub(r"\bint\b", "", body.replace(";", ",")).split(",") if f.strip()]
    assert fields == [f[0] for f in _lib.maa_glow_config._fields_]
    assert all(f[1] is ctypes.c_int for f in _lib.maa_glow_config._fields_)
    assert ctypes.sizeof(_lib.maa_glow_config) == 12 * 4
    from audiogpt_amd import backend
    assert list(backend.GLOW_FIELDS) == fields


def test_library_refusals_by_message_with_a_null_context(lib):
    from audiogpt_amd import _lib, backend
    h = ctypes.c_void_p()
    cfg = backend.glow_config(C.GENERSPEECH_POST_GLOW)

    def create(c, out=h):
        st = lib.maa_glow_create(None, ctypes.byref(c) if c is not None else None, None, 0, ctypes.byref(out) if out is not None else None)
        assert st < 0
        return lib.maa_last_error()

    assert b"null pointer" in create(None)
    assert b"null pointer" in create(cfg, None)
    assert b"null context" in create(cfg)                       # past every configuration check
    for field, bad, message in (("n_sqz", 1, b"n_sqz must be 2"), ("n_sqz", 3, b"n_sqz must be 2"), ("n_split", 2, b"n_split must be 4"),
                                ("n_split", 8, b"n_split must be 4"), ("kernel_size", 4, b"kernel_size must be odd"),
                                ("hidden_channels", 127, b"hidden_channels must be even"),
                                ("hidden_channels", 130, b"hidden_channels must be a multiple of 4"),
                                ("in_channels", 78, b"in_channels % 4 != 0"), ("gin_channels", 1102, b"gin_channels"),
                                ("gin_channels", -4, b"gin_channels"), ("n_blocks", -1, b"bad Glow config"),
                                ("share_wn_layers", -1, b"share_wn_layers")):
        c = backend.glow_config(C.GENERSPEECH_POST_GLOW)
        setattr(c, field, bad)
        assert message in create(c), (field, bad, lib.maa_last_error())
    # the tensor list is read after the context: a null list of one tensor still ends at the context
    assert lib.maa_glow_create(None, ctypes.byref(cfg), None, 1, ctypes.byref(h)) < 0 and b"null context" in lib.maa_last_error()
    buf = np.zeros(256, np.float32)
    dp = buf.ctypes.data + (-buf.ctypes.data) % 64

    def reverse(glow=dp, z=dp + 64, g=dp + 128, mask=None, B=1, T=8, x=dp + 192):
        assert lib.maa_glow_reverse(None, glow, z, g, mask, B, T, x, None, None) < 0
        return lib.maa_last_error()

    assert b"null context" in reverse()
    assert b"null context" in reverse(g=None)                 # d_g against gin_channels needs the handle: after the context
    assert b"null context" in reverse(T=1)                    # T < 2 likewise
    for kw in (dict(glow=None), dict(z=None), dict(x=None)):
        assert b"null pointer" in reverse(**kw), kw
    for kw in (dict(B=0), dict(T=0), dict(B=-1), dict(B=1 << 12, T=1 << 12)):
        assert b"B, T" in reverse(**kw), kw
    assert lib.maa_glow_destroy(None) == 0


def test_zero_config_selects_the_shipped_sizes(lib):
    """A zero in a size field is GenerSpeech's shipped value (include/maa.h): the all-zero structure passes every check, and a
    field that is wrong on its own is still refused beside zeros."""
    from audiogpt_amd import _lib
    h = ctypes.c_void_p()
    zero = _lib.maa_glow_config()
    assert lib.maa_glow_create(None, ctypes.byref(zero), None, 0, ctypes.byref(h)) < 0 and b"null context" in lib.maa_last_error()
    for field, bad, message in (("n_sqz", 1, b"n_sqz"), ("kernel_size", 2, b"kernel_size"), ("in_channels", 6, b"in_channels")):
        c = _lib.maa_glow_config()
        setattr(c, field, bad)
        assert lib.maa_glow_create(None, ctypes.byref(c), None, 0, ctypes.byref(h)) < 0 and message in lib.maa_last_error()
    src = open(os.path.join(ROOT, "include", "maa.h")).read()
    assert "(80, 128, 3, 1, 8, 3, 4, 2)" in src
    GS = C.GENERSPEECH_POST_GLOW
    assert tuple(GS[k] for k in ("in_channels", "hidden_channels", "kernel_size", "dilation_rate", "n_blocks", "n_layers", "n_split",
                                 "n_sqz")) == (80, 128, 3, 1, 8, 3, 4, 2)


def test_postglow_draw_consumes_the_global_generator_as_the_reference_does():
    """PostGlow.infer without z: Normal(0, 1).sample([B, 80, T]) on the host's global generator, times noise_scale -- the latent the
    flow receives is the golden's z and the generator ends where the reference's call leaves it.  The device call is replaced."""
    from audiogpt_amd.generspeech import PostGlow
    g = np.load(os.path.join(GOLDEN, "postglow_gs_t40.npz"))
    seen = {}

    class Net:
        def reverse(self, z, cond, mask, return_logdet=True, return_hiddens=False):
            seen.update(z=z.clone(), cond=cond.clone(), mask=mask)
            return z, None, None

    post = PostGlow.__new__(PostGlow)
    post.cfg, post.device = dict(C.GENERSPEECH_POST_GLOW), torch.device("cpu")
    post.post_flow = type("F", (), {"net": Net()})()
    t = lambda k: torch.from_numpy(g[k])          # noqa: E731
    torch.manual_seed(int(g["draw_seed"]))
    out = post.infer(t("mel_out"), t("decoder_inp"), t("spk_embed"), t("emo_embed"), t("ref_prosody"))
    after = torch.get_rng_state()
    torch.manual_seed(int(g["draw_seed"]))
    ref = torch.distributions.Normal(0, 1).sample((1, 80, 40)) * 0.8
    assert torch.equal(torch.get_rng_state(), after)
    assert torch.equal(seen["z"], ref.transpose(1, 2)) and torch.equal(seen["z"], t("z").transpose(1, 2)) and seen["mask"] is None
    assert out.shape == (1, 40, 80)
    want = R.post_glow_cond(post.cfg, t("mel_out"), t("decoder_inp"), t("spk_embed"), t("emo_embed"), t("ref_prosody"))
    assert torch.equal(seen["cond"], want.transpose(1, 2)) and seen["cond"].shape == (1, 40, 1104)
    # a caller's z: no draw
    torch.manual_seed(7)
    before = torch.get_rng_state()
    post.infer(t("mel_out"), t("decoder_inp"), t("spk_embed"), t("emo_embed"), t("ref_prosody"), z=t("z"))
    assert torch.equal(torch.get_rng_state(), before)


def test_glow_kernels_do_not_spill(tmp_path):
    """vgpr_spill_count and the scratch size of every kernel of glow.hip in the cross-compiled gfx950 assembly's metadata (read as
    tests/test_pe_host.py reads pitch.hip's)."""
    import subprocess
    from audiogpt_amd.build import FLAGS
    csrc = os.path.join(ROOT, "audiogpt_amd", "csrc")
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path / "glow.s")
    cmd = [hipcc] + [f for f in FLAGS if f != "-fPIC"] + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                                                          os.path.join(csrc, "glow.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(out).read()
    meta = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                                 r"\s+\.vgpr_spill_count:\s+(\d+)", text)}
    names = " ".join(meta)
    for k in ("glow_squeeze_kernel", "glow_gate_kernel", "glow_wn_residual_kernel", "glow_block_tail_kernel", "glow_logdet_kernel"):
        assert k in names, k
    assert len(meta) == 5
    for name, (scratch, vg, spill) in meta.items():
        assert spill == 0 and scratch == 0, (name, scratch, spill)
        assert vg <= 128, (name, vg)          # four waves per SIMD: these kernels hide latency by occupancy
