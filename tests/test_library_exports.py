"""CPU-side checks of the C-ABI boundary: the library builds, loads and exports every symbol that
include/maa.h declares (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from audiogpt_amd import build
    return build.build(verbose=False)


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "maa.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(maa_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported(lib_path):
    lib = ctypes.CDLL(lib_path)
    syms = _declared_symbols()
    assert len(syms) >= 25
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_binding_matches_header(lib_path):
    from audiogpt_amd import _lib
    assert sorted(_lib.EXPORTS) == _declared_symbols()
    lib = _lib.load()
    assert b"gfx950" in lib.maa_version()


def _declared_argument_counts():
    """{entry: number of parameters} of every status-returning entry include/maa.h declares."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(maa_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


def test_every_bound_signature_has_the_headers_argument_count(lib_path):
    """The binding's one table (_lib.SIGNATURES) against the header, entry by entry: the same names, and as many argument types
    as the declaration has parameters."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    declared = _declared_argument_counts()
    assert sorted(declared) == sorted(_lib.SIGNATURES) and len(declared) >= 80
    assert sorted(_lib.EXPORTS) == sorted(list(_lib.SIGNATURES) + ["maa_last_error", "maa_version"])
    for name, n in declared.items():
        assert len(_lib.SIGNATURES[name]) == n, name
        assert len(getattr(lib, name).argtypes) == n and getattr(lib, name).restype is ctypes.c_int, name


def test_error_path_without_gpu(lib_path):
    """No GPU in the build container: creating a context must fail cleanly with a message, not crash."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from audiogpt_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    st = lib.maa_ctx_create(0, None, ctypes.byref(h))
    assert st < 0
    assert len(lib.maa_last_error()) > 0
    from audiogpt_amd import backend
    with pytest.raises(_lib.MaaError):
        backend.Context("cuda:0")


def test_null_arguments_are_rejected(lib_path):
    from audiogpt_amd import _lib
    lib = _lib.load()
    assert lib.maa_ctx_synchronize(None) < 0
    assert lib.maa_unet_forward(None, None, None, None, 1, 1, 1, None) < 0
    assert lib.maa_vocoder_forward(None, None, None, 1, 1, None) < 0
    assert b"null" in lib.maa_last_error() or b"bad" in lib.maa_last_error()


def test_normalisation_test_entries_are_bound_and_reject_null(lib_path):
    """maa_op_groupnorm_ex / maa_op_layernorm_ex / maa_op_split32 (tests/test_gpu_norm_ops.py) are declared, exported, bound
    with the header's argument counts, and fail with a message on null arguments."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    for name in ("maa_op_groupnorm_ex", "maa_op_layernorm_ex", "maa_op_split32"):
        assert name in _lib.EXPORTS and name in _declared_symbols()
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(getattr(lib, name).argtypes) == len(decl.split(",")), name
    assert lib.maa_op_groupnorm_ex(None, None, 0, 0, None, 0, 0, 1, 1, 32, None, None, 1e-5, 0, None, 0, None) < 0
    assert lib.maa_op_layernorm_ex(None, None, 1, 4, None, None, 1e-5, None, 0) < 0
    assert lib.maa_op_split32(None, None, 1, 32, 1.0, 0, None) < 0
    assert len(lib.maa_last_error()) > 0


def test_sequence_row_test_entry_is_bound_and_refuses_by_name(lib_path):
    """maa_op_seq_rows (tests/test_gpu_seq_ops.py) is declared, exported, bound with the header's argument count and a structure
    that has the header's fields in the header's order, and every refusal -- null pointers, C % 4, the head's width, the GroupNorm
    channel rule, rows < 1, table_rows < 2 -- comes back with its message before the context is touched."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    name = "maa_op_seq_rows"
    assert name in _lib.EXPORTS and name in _declared_symbols()
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    assert len(getattr(lib, name).argtypes) == len(decl.split(",")) == 2, name
    body = re.search(r"typedef struct \{([^}]*)\} maa_seq_rows_args;", src).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?(float|int)\s*\*?", "", stmt).split(",")]
    assert fields == [f[0] for f in _lib.maa_seq_rows_args._fields_]
    for kind, value in _lib.SEQ_KINDS.items():
        assert re.search(r"#define MAA_SEQ_%s %d\b" % (kind.upper(), value), src), kind
    assert lib.maa_op_seq_rows(None, None) < 0 and b"null pointer" in lib.maa_last_error()
    import numpy as np
    buf = np.zeros(64, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    dp = buf.ctypes.data
    base = {
        "frame_mask": dict(rows=1, C=8, d_x=dp, d_out=dp),
        "affine_mask": dict(rows=1, C=8, d_x=dp, d_mask=dp, d_out=dp),
        "gn_relu_res": dict(B=1, T=1, C=8, d_x=dp, d_res=dp, h_gamma=fp, h_beta=fp, groups=2, eps=1e-5, d_out=dp),
        "pos_add": dict(B=1, T=1, C=8, d_x=dp, table_rows=2, alpha=1.0, d_out=dp),
        "head": dict(rows=1, C=8, d_x=dp, d_mask=dp, h_gamma=fp, h_beta=fp, h_w=fp, h_bias=fp, eps=1e-5, n_out=2, d_out=dp, d_out2=dp),
    }

    def refused(kind, message, **kw):
        d = dict(base[kind], kind=_lib.SEQ_KINDS[kind])
        d.update(kw)
        st = lib.maa_op_seq_rows(None, ctypes.byref(_lib.maa_seq_rows_args(**d)))
        assert st < 0 and message in lib.maa_last_error(), (kind, kw, lib.maa_last_error())

    for kind in base:
        refused(kind, b"null context")                                  # past every argument check
        for p in [k for k, v in base[kind].items() if k.startswith(("d_", "h_"))]:
            refused(kind, b"null pointer", **{p: None})
        refused(kind, b"C % 4 != 0", C=6)
        refused(kind, b"C % 4 != 0", C=0)
        if "rows" in base[kind]:
            refused(kind, b"rows < 1", rows=0)
        else:
            refused(kind, b"rows < 1", B=0)
            refused(kind, b"rows < 1", T=0)
    refused("head", b"null context", n_out=1, d_out2=None, d_dur=dp)
    refused("head", b"null pointer", n_out=1)                            # the duration head writes d_dur
    refused("head", b"head C > 1024", C=1028)
    refused("head", b"n_out", n_out=3)
    refused("affine_mask", b"both or neither", h_scale=fp)
    refused("affine_mask", b"null context", h_scale=fp, h_shift=fp)
    for bad in (dict(groups=0), dict(groups=3), dict(groups=8), dict(C=1024, groups=2)):      # 0, not a divisor, 1 per group, 512
        refused("gn_relu_res", b"groups", **bad)
    refused("pos_add", b"table_rows < 2", table_rows=1)
    refused("pos_add", b"null context", d_pos=dp)
    assert lib.maa_op_seq_rows(None, ctypes.byref(_lib.maa_seq_rows_args(kind=5))) < 0 and b"unknown kind" in lib.maa_last_error()


def test_tts_row_test_entry_is_bound_and_refuses_by_name(lib_path):
    """maa_op_tts_rows (tests/test_gpu_tts_ops.py) is declared, exported, bound with the header's argument count and a structure
    that has the header's fields in the header's order, with the header's types; the kinds' #defines match; a null structure, an
    unknown kind and every host-side refusal come back with their message before the context is touched."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    name = "maa_op_tts_rows"
    assert name in _lib.EXPORTS and name in _declared_symbols()
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    assert len(getattr(lib, name).argtypes) == len(decl.split(",")) == 2, name
    body = re.search(r"typedef struct \{([^}]*)\} maa_tts_rows_args;", src).group(1)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            m = re.match(r"^(const\s+)?(float|int)\s*(\*?)\s*(.*)$", stmt)
            pointer = (ctypes.POINTER(ctypes.c_float) if m.group(4).startswith("h_") else ctypes.c_void_p) if m.group(3) else None
            fields += [(f.strip(), pointer or ctype[m.group(2)]) for f in m.group(4).split(",")]
    assert fields == list(_lib.maa_tts_rows_args._fields_)

    class Mirror(ctypes.Structure):          # the header's fields under the C layout rules
        _fields_ = fields
    assert ctypes.sizeof(Mirror) == ctypes.sizeof(_lib.maa_tts_rows_args) == 14 * 4 + 2 * 4 + 28 * 8
    for kind, value in _lib.TTS_KINDS.items():
        assert re.search(r"#define MAA_TTS_%s %d\b" % (kind.upper(), value), src), kind
    assert sorted(_lib.TTS_KINDS.values()) == list(range(10))
    assert not re.search(r"#define MAA_SEQ_\w+ [5-9]\b", src)                 # nothing was added to maa_op_seq_rows
    assert lib.maa_op_tts_rows(None, None) < 0 and b"null pointer" in lib.maa_last_error()
    import numpy as np
    buf = np.zeros(64, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    dp = buf.ctypes.data                                     # stands in for device memory; never read
    base = {
        "glow_squeeze": dict(B=1, T=2, C=8, d_x=dp, d_out=dp),
        "glow_gate": dict(rows=1, C=8, d_x=dp, d_out=dp),
        "glow_wn_residual": dict(rows=1, C=8, d_x=dp, d_mask=dp, first=1, last=0, d_out=dp, d_out2=dp),
        "glow_block_tail": dict(rows=1, C=8, d_x=dp, d_y=dp, d_mask=dp, h_winv=fp, h_an_bias=fp, h_an_einv=fp, first=1, d_out=dp,
                                d_rowld=dp),
        "glow_logdet": dict(B=1, T=1, d_x=dp, d_mask=dp, alpha=1.0, d_out=dp),
        "fs2_embed_plain": dict(B=1, T=3, C=8, d_tok=dp, h_table=fp, vocab=4, h_pe=fp, pe_rows=4, alpha=1.0, d_out=dp, d_out2=dp,
                                d_out3=dp),
        "fs2_add_speaker": dict(B=1, T=3, C=8, d_x=dp, d_spk=dp, d_mask=dp, d_out=dp),
        "fs2_speaker_gather": dict(B=2, C=8, h_table=fp, h_t1=fp, h_t2=fp, n_rows=2, d_out=dp),
        "fs2_energy_tail": dict(rows=6, T=3, C=8, H=8, d_x=dp, h_gamma=fp, h_beta=fp, h_w=fp, h_bias=fp, eps=1e-5, d_mel2ph=dp, d_y=dp,
                                h_table=fp, d_out=dp),
        "fs2_tgt_mask": dict(rows=1, d_mel2ph=dp, d_out=dp),
    }
    assert sorted(base) == sorted(_lib.TTS_KINDS)

    def refused(kind, message, **kw):
        d = dict(base[kind], kind=_lib.TTS_KINDS[kind])
        d.update(kw)
        st = lib.maa_op_tts_rows(None, ctypes.byref(_lib.maa_tts_rows_args(**d)))
        assert st < 0 and message in lib.maa_last_error(), (kind, kw, lib.maa_last_error())

    for kind in base:
        refused(kind, b"null context")                                  # past every argument check
        for p in [k for k in base[kind] if k.startswith(("d_", "h_"))]:
            if (kind, p) != ("fs2_energy_tail", "d_x"):                 # (the tail's d_x is nullable: the form without a branch)
                refused(kind, b"null pointer", **{p: None})
        if "C" in base[kind]:
            refused(kind, b"C % 4 != 0", C=6)
            refused(kind, b"C % 4 != 0", C=0)
        if "rows" in base[kind]:
            refused(kind, b"rows < 1", rows=0)
        else:
            refused(kind, b"rows < 1", B=0)
        if "T" in base[kind] and "rows" not in base[kind]:
            refused(kind, b"rows < 1", T=0)
    # every nullable pointer may be given
    refused("glow_squeeze", b"null context", d_mask=dp, d_out2=dp)
    refused("glow_block_tail", b"null context", d_h_cpl=dp, d_h_inv=dp, d_h_act=dp)
    refused("fs2_add_speaker", b"null context", d_mask=None, d_mel2ph=dp)
    refused("fs2_speaker_gather", b"null context", d_ids=dp, split=1, n_rows=1)
    refused("fs2_energy_tail", b"null context", d_energy=dp, d_spk=dp, d_energy_pred=dp, d_bin=dp)
    refused("fs2_energy_tail", b"null context", d_x=None, C=0, h_gamma=None, h_beta=None, h_w=None, h_bias=None, h_table=None)
    # the kinds' own rules
    refused("glow_squeeze", b"T < 2", T=1)
    refused("glow_wn_residual", b"0 or 1", last=2)
    refused("glow_wn_residual", b"0 or 1", first=-1)
    refused("glow_block_tail", b"0 or 1", sigmoid_scale=2)
    refused("fs2_embed_plain", b"rel is 0 or 1", rel=2)
    refused("fs2_embed_plain", b"vocab < 1", vocab=0)
    refused("fs2_embed_plain", b"pe_rows too small", pe_rows=3)
    refused("fs2_embed_plain", b"null context", pe_rows=3, rel=1)
    refused("fs2_add_speaker", b"not both", d_mel2ph=dp)
    refused("fs2_speaker_gather", b"split is 0 or 1", split=2)
    refused("fs2_speaker_gather", b"n_rows", n_rows=1)                    # without ids row b is read: n_rows >= B
    refused("fs2_speaker_gather", b"n_rows", n_rows=0, d_ids=dp)
    refused("fs2_energy_tail", b"H % 4 != 0", H=6)
    refused("fs2_energy_tail", b"rows % T != 0", rows=7)
    refused("fs2_energy_tail", b"rows % T != 0", T=0)
    refused("fs2_energy_tail", b"C > 1024", C=1028)
    refused("fs2_energy_tail", b"eps", eps=0.0)
    for kind in (-1, 10):
        assert lib.maa_op_tts_rows(None, ctypes.byref(_lib.maa_tts_rows_args(kind=kind))) < 0
        assert b"unknown kind" in lib.maa_last_error()


def test_sampler_step_test_entry_is_bound_and_refuses_by_name(lib_path):
    """maa_op_sampler_step (tests/test_gpu_sampler_ops.py) is declared, exported, bound with the header's argument count and a
    structure that has the header's fields in the header's order and the size the header's types give, and every host-side refusal
    comes back with its own message before the context is touched."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    name = "maa_op_sampler_step"
    assert name in _lib.EXPORTS and name in _declared_symbols()
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    assert len(getattr(lib, name).argtypes) == len(decl.split(",")) == 2, name
    body = re.search(r"typedef struct \{([^}]*)\} maa_sampler_step_args;", src).group(1)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "int64_t": ctypes.c_int64}
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            m = re.match(r"^(?:const\s+)?(float|int64_t|int)\s*(\*?)\s*(.*)$", stmt)
            fields += [(f.strip(), ctypes.c_void_p if m.group(2) else ctype[m.group(1)]) for f in m.group(3).split(",")]
    assert fields == list(_lib.maa_sampler_step_args._fields_)

    class Mirror(ctypes.Structure):          # the header's fields under the C layout rules
        _fields_ = fields
    assert ctypes.sizeof(Mirror) == ctypes.sizeof(_lib.maa_sampler_step_args) == 16 + 3 * 8 + 2 * 4 + 8 * 4 + 23 * 8
    for kind, value in _lib.STEP_KINDS.items():
        assert re.search(r"#define MAA_STEP_%s %d\b" % (kind.upper(), value), src), kind
    assert len(set(_lib.STEP_KINDS.values())) == 9
    assert lib.maa_op_sampler_step(None, None) < 0 and b"null pointer" in lib.maa_last_error()
    import numpy as np
    buf = np.zeros(256, np.float32)
    dp = buf.ctypes.data + (-buf.ctypes.data) % 16          # stands in for device memory; never read
    ldm = dict(B=2, nB=4, S=4, n=16, per=8, per_in=8, scale=3.0, temperature=1.0)
    base = {
        "ddim_prepare": dict(ldm, d_x=dp, d_tab_t=dp, d_tab=dp, d_step=dp, d_xin=dp, d_cur_t=dp, d_coef=dp),
        "ddim": dict(ldm, d_xin=dp, d_eps_u=dp, d_coef=dp, d_x=dp, d_step=dp),
        "plms": dict(ldm, d_xin=dp, d_eps_u=dp, d_coef=dp, d_x=dp, d_step=dp, d_ring=dp),
        "plms_euler_mid": dict(ldm, d_xin=dp, d_eps_u=dp, d_coef=dp, d_x=dp, d_e_keep=dp, d_tab_t=dp, d_cur_t=dp),
        "plms_euler_final": dict(ldm, d_eps_u=dp, d_coef=dp, d_x=dp, d_e_keep=dp, d_step=dp),
        "ddpm": dict(ldm, d_xin=dp, d_eps_u=dp, d_coef=dp, d_tab=dp, d_x=dp, d_noise_p=dp, d_step=dp),
        "ds_plms": dict(n=16, interval=10, mode=0, d_x=dp, d_eps_u=dp, d_ring=dp, d_tab=dp, d_st=dp),
        "ds_advance": dict(B=2, interval=10, d_st=dp, d_cur_t=dp),
        "ds_ddpm": dict(n=16, timesteps=5, n_steps=5, start=4, d_x=dp, d_eps_u=dp, d_noise_p=dp, d_tab=dp, d_st=dp),
    }
    assert sorted(base) == sorted(_lib.STEP_KINDS)

    def refused(kind, message, **kw):
        d = dict(base[kind], kind=_lib.STEP_KINDS[kind])
        d.update(kw)
        st = lib.maa_op_sampler_step(None, ctypes.byref(_lib.maa_sampler_step_args(**d)))
        assert st < 0 and message in lib.maa_last_error(), (kind, kw, lib.maa_last_error())

    rows = ("ddim_prepare", "ddim", "plms", "plms_euler_mid", "ddpm")
    for kind in base:
        refused(kind, b"null context")                                  # past every argument check
        for p in [k for k in base[kind] if k.startswith("d_")]:
            refused(kind, b"null pointer", **{p: None})
        if kind in rows:
            refused(kind, b"B < 1", B=0)
            refused(kind, b"per < 1", per=0)
            refused(kind, b"per < 1", per_in=4)
            refused(kind, b"n % per != 0", n=17)
            refused(kind, b"n % per != 0", n=24)
        elif kind != "ds_advance":
            refused(kind, b"n < 1", n=0)
    for kind in ("ddim_prepare", "plms_euler_mid"):
        refused(kind, b"nB is B or 2 B", nB=3)
        refused(kind, b"null context", nB=2)
        refused(kind, b"nB > 256", B=129, nB=258, n=129 * 8)
        refused(kind, b"null pointer", d_emb_tab=dp)                      # an embedding table needs its slot
        refused(kind, b"null context", d_emb_tab=dp, d_cur_emb=dp, emb_w=4)
    refused("ddim_prepare", b"null pointer", per_in=12)                   # concat channels need d_concat
    refused("ddim_prepare", b"null context", per_in=12, d_concat=dp)
    for kind in ("ddim_prepare", "ddim", "plms"):
        refused(kind, b"S < 1", S=0)
    for kind in ("ddim_prepare", "ddpm"):
        refused(kind, b"mask given without x0", d_mask=dp)
        refused(kind, b"mask given without x0", d_mask=dp, d_x0=dp)
        refused(kind, b"null context", d_mask=dp, d_x0=dp, d_noise_q=dp)
    for kind in ("ddim", "plms", "plms_euler_final", "ddpm"):
        refused(kind, b"both or neither", d_log_x=dp)
        refused(kind, b"null context", d_log_x=dp, d_log_x0=dp)
    refused("ds_plms", b"mode outside 0..2", mode=3)
    refused("ds_plms", b"mode outside 0..2", mode=-1)
    refused("ds_plms", b"mode 2 needs e_prev", mode=2)
    refused("ds_plms", b"mode 1 needs x_out", mode=1)
    refused("ds_plms", b"null context", mode=2, d_e_prev=dp)
    refused("ds_plms", b"null context", mode=1, d_x_out=dp)
    refused("ds_plms", b"interval < 1", interval=0)
    refused("ds_advance", b"interval < 1", interval=0)
    refused("ds_advance", b"B < 1", B=0)
    refused("ds_advance", b"B > 256", B=257)
    refused("ds_advance", b"null context", B=256)
    refused("ds_ddpm", b"timesteps or n_steps < 1", timesteps=0)
    refused("ds_ddpm", b"whole aligned float4s", n=18)
    refused("ds_ddpm", b"whole aligned float4s", d_x=dp + 4)
    for kind in (-1, 9):
        assert lib.maa_op_sampler_step(None, ctypes.byref(_lib.maa_sampler_step_args(kind=kind))) < 0
        assert b"unknown kind" in lib.maa_last_error()


def test_front_rows_test_entry_is_bound_and_refuses_by_name(lib_path):
    """maa_op_front_rows (tests/test_gpu_frontend_ops.py) is declared, exported, bound with the header's argument count and a
    structure that has the header's fields in the header's order and the size the header's types give, the kinds' #defines match,
    and every host-side refusal comes back with its own message before the context is touched."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    name = "maa_op_front_rows"
    assert name in _lib.EXPORTS and name in _declared_symbols()
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    assert len(getattr(lib, name).argtypes) == len(decl.split(",")) == 2, name
    body = re.search(r"typedef struct \{([^}]*)\} maa_front_rows_args;", src).group(1)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            m = re.match(r"^(const\s+)?(float|int)\s*(\*?)\s*(.*)$", stmt)
            pointer = (ctypes.POINTER(ctypes.c_float) if m.group(4).startswith("h_") else ctypes.c_void_p) if m.group(3) else None
            fields += [(f.strip(), pointer or ctype[m.group(2)]) for f in m.group(4).split(",")]
    assert fields == list(_lib.maa_front_rows_args._fields_)

    class Mirror(ctypes.Structure):          # the header's fields under the C layout rules
        _fields_ = fields
    assert ctypes.sizeof(Mirror) == ctypes.sizeof(_lib.maa_front_rows_args) == 20 * 4 + 2 * 4 + 4 * 8
    for kind, value in _lib.FRONT_KINDS.items():
        assert re.search(r"#define MAA_FRONT_%s %d\b" % (kind.upper(), value), src), kind
    assert sorted(_lib.FRONT_KINDS.values()) == [0, 1, 2, 3, 4]
    assert lib.maa_op_front_rows(None, None) < 0 and b"null pointer" in lib.maa_last_error()
    import numpy as np
    buf = np.zeros(64, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    dp = buf.ctypes.data                                     # stands in for device memory; never read
    base = {
        "pad": dict(B=2, n=8, left=3, total=16, ldo=20, mode=1, d_x=dp, d_out=dp),
        "power": dict(rows=2, nf=5, ldy=10, ldm=8, power2=1, d_x=dp, d_out=dp),
        "logmel": dict(B=1, frames=2, n_mels=8, ldmel=8, log_kind=0, layout=1, amin=1e-10, ref_db=0.0, d_x=dp, d_out=dp),
        "affine": dict(n=16, F=8, d_x=dp, h_scale=fp, h_shift=fp, d_out=dp),
        "pool": dict(B=1, T=2, F=2, C=4, d_x=dp, d_out=dp),
    }
    assert sorted(base) == sorted(_lib.FRONT_KINDS)

    def refused(kind, message, **kw):
        d = dict(base[kind], kind=_lib.FRONT_KINDS[kind])
        d.update(kw)
        st = lib.maa_op_front_rows(None, ctypes.byref(_lib.maa_front_rows_args(**d)))
        assert st < 0 and message in lib.maa_last_error(), (kind, kw, lib.maa_last_error())

    for kind in base:
        refused(kind, b"null context")                                  # past every argument check
        for p in [k for k in base[kind] if k.startswith(("d_", "h_"))]:
            refused(kind, b"null pointer", **{p: None})
    for kind, sizes in (("pad", "B n"), ("power", "rows nf"), ("logmel", "B frames n_mels"), ("affine", "n F"), ("pool", "B T F C")):
        for s in sizes.split():
            for bad in (0, -1):
                refused(kind, ("op_front_rows: %s < 1" % s).encode(), **{s: bad})
    refused("pad", b"total < left + n", total=10)
    refused("pad", b"null context", total=11, ldo=11, mode=0)
    refused("pad", b"ldo < total", ldo=15)
    refused("pad", b"null context", ldo=16)
    refused("pad", b"left < 0", left=-1)
    refused("pad", b"unknown mode", mode=2)
    refused("pad", b"unknown mode", mode=-1)
    refused("pad", b"reflect padding needs a signal longer than the pad", left=8, total=20)          # n == left
    refused("pad", b"reflect padding needs a signal longer than the pad", left=0)                    # n == right
    refused("pad", b"null context", left=7, total=16, ldo=16)                                         # n = left + 1 = right + 7
    refused("pad", b"null context", left=8, total=20, mode=0)                                         # zeros take any widths
    refused("power", b"ldy < 2 nf", ldy=9)
    refused("power", b"ldm < nf", ldm=4)
    refused("power", b"null context", ldm=5, power2=0)
    refused("logmel", b"ldmel < n_mels", ldmel=7)
    refused("logmel", b"null context", ldmel=11, log_kind=1, layout=0, amin=1e-5)
    refused("logmel", b"amin <= 0", amin=0.0)
    refused("logmel", b"amin <= 0", amin=-1.0)
    refused("logmel", b"unknown log_kind", log_kind=2)
    refused("logmel", b"unknown layout", layout=2)
    refused("logmel", b"unknown layout", layout=-1)
    for kind in (-1, 5):
        assert lib.maa_op_front_rows(None, ctypes.byref(_lib.maa_front_rows_args(kind=kind))) < 0
        assert b"unknown kind" in lib.maa_last_error()


def test_contraction_test_entry_is_bound_and_rejects_null(lib_path):
    """maa_op_igemm_ex (tests/test_gpu_igemm_ops.py) is declared, exported, bound with the header's argument count and a structure
    that has the header's fields in the header's order, and fails with a message on null arguments, on a pitch below its width and
    on presplit outside its preconditions -- all checked before the context is touched."""
    from audiogpt_amd import _lib
    lib = _lib.load()
    raw = open(os.path.join(ROOT, "include", "maa.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    name = "maa_op_igemm_ex"
    assert name in _lib.EXPORTS and name in _declared_symbols()
    decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
    assert len(getattr(lib, name).argtypes) == len(decl.split(",")), name
    body = re.search(r"typedef struct \{([^}]*)\} maa_igemm_ex_args;", src).group(1)
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            fields += [f.strip().lstrip("*").strip() for f in re.sub(r"^(const\s+)?(float|int)\s*\*?", "", stmt).split(",")]
    assert fields == [f[0] for f in _lib.maa_igemm_ex_args._fields_]
    assert lib.maa_op_igemm_ex(None, None) < 0 and b"null pointer" in lib.maa_last_error()
    import numpy as np
    buf = np.zeros(64, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def args(**kw):      # a 1x1 convolution 32 -> 32 on a 1x1 image; the buffer stands in for device memory and is never read
        d = dict(d_x1=buf.ctypes.data, ld1=32, C1=32, B=1, H=1, W=1, Ho=1, Wo=1, h_w=fp, Cout=32, KH=1, KW=1, stride=1, dil=1,
                 pad_h=-1, alpha=1.0, out_scale=1.0, d_c=buf.ctypes.data, ldc=32)
        d.update(kw)
        return ctypes.byref(_lib.maa_igemm_ex_args(**d))

    assert lib.maa_op_igemm_ex(None, args()) < 0 and b"null context" in lib.maa_last_error()      # past every argument check
    for bad in (dict(ldc=31), dict(ld1=31), dict(d_res=buf.ctypes.data, ldr=16), dict(d_c2=buf.ctypes.data, ldc2=0),
                dict(d_rowadd=buf.ctypes.data, ld_rowadd=8), dict(d_x2=buf.ctypes.data, C2=8, ld2=4)):
        assert lib.maa_op_igemm_ex(None, args(**bad)) < 0 and b"pitch" in lib.maa_last_error(), bad
    for bad in (dict(B=0), dict(Cout=0), dict(stride=0), dict(pad_h=-2)):
        assert lib.maa_op_igemm_ex(None, args(**bad)) < 0 and b"sizes" in lib.maa_last_error(), bad
    assert lib.maa_op_igemm_ex(None, args(C2=8)) < 0 and b"second source" in lib.maa_last_error()
    assert lib.maa_op_igemm_ex(None, args(geglu=1)) < 0 and b"GEGLU" in lib.maa_last_error()
    for bad in (dict(C1=16, ld1=16), dict(ld1=64), dict(d_x2=buf.ctypes.data, C2=32, ld2=32)):
        assert lib.maa_op_igemm_ex(None, args(presplit=1, **bad)) < 0 and b"presplit" in lib.maa_last_error(), bad
