"""Every entry of the C ABI checks its arguments before it touches the context (csrc/api.cpp: checks, bind, work), so without a
device a malformed call is refused by an argument check and a well-formed one by the missing context.  The well-formed calls
pass host buffers that stand in for device memory and fake handles: neither is ever read, the context is null."""
import ctypes as C

import numpy as np
import pytest

from audiogpt_amd import _lib as L

# the entries the rule cannot show on, each with the reason (read off csrc/api.cpp)
EXCEPTIONS = {
    "maa_ctx_create": "makes the context; its one check, of device_id, needs the device count",
    "maa_ctx_destroy": "the context is its only argument (null is a no-op)",
    "maa_ctx_synchronize": "the context is its only argument",
    "maa_ctx_reload_tuning": "the context is its only argument",
    "maa_prof_begin": "beside the context it takes a flag, and every value of it is valid: there is nothing to refuse",
}
EXCEPTIONS.update({name: "takes the handle alone, no context; null is a no-op" for name in L.SIGNATURES if name.endswith("_destroy")
                   and name != "maa_ctx_destroy"})
# malformed calls are all-null / all-zero; where zero is a valid value of the only checked argument, an invalid one
MALFORMED = {"maa_ctx_set_precision": (3,), "maa_ctx_set_cfg_split": (2,)}

_buf = np.zeros(4096, np.float32)
_base = _buf.ctypes.data + (-_buf.ctypes.data) % 64          # 64-byte aligned stand-in for device memory
_fp = C.cast(_base, C.POINTER(C.c_float))
_keep = []


def _struct(t, **kw):
    s = t(**kw)
    _keep.append(s)
    return C.byref(s)


def _ddim_args():
    ts = (C.c_int32 * 2)(1, 0)
    _keep.append(ts)
    return dict(S=2, B=1, C=4, H=10, W=78, scale=1.0, h_timesteps=ts, h_alphas=_fp, h_alphas_prev=_fp, temperature=1.0)


def _configs():
    from audiogpt_amd import backend, config
    voc = L.maa_vocoder_config(num_mels=80, upsample_initial_channel=32, n_upsamples=1, n_kernels=1, n_dilations=1, resblock=1)
    voc.upsample_rates[0], voc.upsample_kernel_sizes[0], voc.resblock_kernel_sizes[0] = 2, 4, 3
    clap = L.maa_clap_audio_config(mel_bins=64, n_blocks=1, out_emb=64, d_proj=64, bn_eps=1e-5)
    clap.channels[0] = 32
    _keep.extend([voc, clap])
    return {
        L.maa_unet_config: _struct(L.maa_unet_config, n_channel_mult=1, model_channels=32),
        L.maa_vae_config: _struct(L.maa_vae_config, n_ch_mult=1),
        L.maa_vocoder_config: C.byref(voc),
        L.maa_diffnet_config: _struct(L.maa_diffnet_config, in_dims=80, hidden_size=256, residual_layers=1, residual_channels=64,
                                      dilation_cycle_length=1),
        L.maa_pitch_extractor_config: _struct_of(backend.pe_config(config.PITCH_EXTRACTOR)),
        L.maa_fs2_config: _struct_of(backend.fs2_config(config.FASTSPEECH2_MIDI)),
        L.maa_fs2_pitch_config: _struct_of(backend.fs2_pitch_config(config.FASTSPEECH2_MIDI_CASCADE)),
        L.maa_encoder_config: _struct(L.maa_encoder_config, kind=0, layers=1, width=64, heads=1, mlp_dim=128, d_proj=64, vocab=16,
                                      max_positions=8, ln_eps=1e-5),
        L.maa_clap_audio_config: C.byref(clap),
        L.maa_spectral_config: _struct(L.maa_spectral_config, n_fft=8, hop=4, n_freq=5, n_mels=2, power=1, amin=1e-5, ref=1.0),
        L.maa_ddim_args: _struct(L.maa_ddim_args, **_ddim_args()),
        L.maa_ddpm_args: _struct(L.maa_ddpm_args, loop=L.maa_ddim_args(d_noise_p=_base, **_ddim_args()), start=1, n=2, h_sqrt_recip_ac=_fp,
                                 h_sqrt_recipm1_ac=_fp, h_coef1=_fp, h_coef2=_fp, h_logvar=_fp),
        L.maa_plms_args: _struct(L.maa_plms_args, B=1, T=8, K_step=10, interval=10, timesteps=10, d_cond=_base, h_alphas_cumprod=_fp),
        L.maa_ds_ddpm_args: _struct(L.maa_ds_ddpm_args, B=1, T=8, start=1, n=2, timesteps=10, d_cond=_base, d_noise=_base,
                                    h_sqrt_recip_ac=_fp, h_sqrt_recipm1_ac=_fp, h_coef1=_fp, h_coef2=_fp, h_sigma=_fp),
        L.maa_igemm_ex_args: _struct(L.maa_igemm_ex_args, d_x1=_base, ld1=32, C1=32, B=1, H=1, W=1, Ho=1, Wo=1, h_w=_fp, Cout=32, KH=1,
                                     KW=1, stride=1, dil=1, pad_h=-1, alpha=1.0, out_scale=1.0, d_c=_base, ldc=32),
        L.maa_seq_rows_args: _struct(L.maa_seq_rows_args, kind=L.SEQ_KINDS["head"], rows=1, C=32, d_x=_base, d_mask=_base, h_gamma=_fp,
                                     h_beta=_fp, h_w=_fp, h_bias=_fp, eps=1e-5, n_out=2, d_out=_base, d_out2=_base),
        L.maa_tts_rows_args: _struct(L.maa_tts_rows_args, **_tts_rows()["glow_block_tail"]),
        L.maa_sampler_step_args: _struct(L.maa_sampler_step_args, kind=L.STEP_KINDS["ddim"], B=1, nB=1, S=2, n=8, per=8, per_in=8,
                                         scale=1.0, temperature=1.0, d_x=_base, d_xin=_base + 256, d_eps_u=_base + 512,
                                         d_coef=_base + 768, d_step=_base + 1024),
        L.maa_front_rows_args: _struct(L.maa_front_rows_args, kind=L.FRONT_KINDS["pad"], B=1, n=8, left=2, total=12, ldo=12, mode=1,
                                       d_x=_base, d_out=_base + 256),
        L.maa_prof_row: C.cast(_base, C.POINTER(L.maa_prof_row)),
        L.maa_tensor: None,          # an empty tensor list, with n_tensors = 0
    }


def _tts_rows():
    """{kind: the fields of a well-formed maa_tts_rows_args} -- one per kind of maa_op_tts_rows."""
    d, h = _base, _fp
    calls = {
        "glow_squeeze": dict(B=1, T=4, C=8, d_x=d, d_mask=d + 256, d_out=d + 512, d_out2=d + 768),
        "glow_gate": dict(rows=2, C=8, d_x=d, d_out=d + 256),
        "glow_wn_residual": dict(rows=2, C=8, d_x=d, d_mask=d + 256, first=0, last=1, d_out=d + 512, d_out2=d + 768),
        "glow_block_tail": dict(rows=2, C=8, d_x=d, d_y=d + 256, d_mask=d + 512, sigmoid_scale=1, h_winv=h, h_an_bias=h, h_an_einv=h,
                                first=0, d_out=d + 768, d_rowld=d + 1024, d_h_cpl=d + 1280, d_h_inv=d + 1536, d_h_act=d + 1792),
        "glow_logdet": dict(B=2, T=3, d_x=d, d_mask=d + 256, alpha=-1.5, d_out=d + 512),
        "fs2_embed_plain": dict(B=2, T=3, C=8, d_tok=d, h_table=h, vocab=5, h_pe=h, pe_rows=4, alpha=2.0, rel=0, d_out=d + 256,
                                d_out2=d + 512, d_out3=d + 768),
        "fs2_add_speaker": dict(B=2, T=3, C=8, d_x=d, d_spk=d + 256, d_mel2ph=d + 512, d_out=d + 768),
        "fs2_speaker_gather": dict(B=2, C=8, h_table=h, h_t1=h, h_t2=h, d_ids=d, split=1, n_rows=3, d_out=d + 256),
        "fs2_energy_tail": dict(rows=6, T=3, C=8, H=12, d_x=d, h_gamma=h, h_beta=h, h_w=h, h_bias=h, eps=1e-5, d_mel2ph=d + 256,
                                d_energy=d + 512, d_y=d + 768, h_table=h, d_spk=d + 1024, d_energy_pred=d + 1280, d_bin=d + 1536,
                                d_out=d + 1792),
        "fs2_tgt_mask": dict(rows=5, d_mel2ph=d, d_out=d + 256),
    }
    return {k: dict(v, kind=L.TTS_KINDS[k]) for k, v in calls.items()}


# one malformed call per kind of maa_op_tts_rows: the field that makes it so
TTS_MALFORMED = {
    "glow_squeeze": dict(T=1), "glow_gate": dict(C=6), "glow_wn_residual": dict(d_out2=None), "glow_block_tail": dict(h_winv=None),
    "glow_logdet": dict(d_mask=None), "fs2_embed_plain": dict(pe_rows=3), "fs2_add_speaker": dict(d_mask=_base + 1280),
    "fs2_speaker_gather": dict(n_rows=0), "fs2_energy_tail": dict(rows=7), "fs2_tgt_mask": dict(rows=0),
}


def _struct_of(s):
    _keep.append(s)
    return C.byref(s)


# arguments (after the context) that the generic choice -- 1 for a number, a buffer for a pointer -- does not satisfy:
# {entry: {position: value}}, NULL for a pointer that has to be null
NULL = object()
WELL_FORMED = {
    "maa_unet_create": {2: 0}, "maa_vae_create": {2: 0}, "maa_vocoder_create": {2: 0}, "maa_diffnet_create": {2: 0},
    "maa_pitch_extractor_create": {2: 0}, "maa_fs2_create": {2: 0}, "maa_fs2_pitch_create": {2: 0}, "maa_encoder_create": {2: 0},
    "maa_clap_audio_create": {2: 0},
    "maa_unet_forward_split": {5: 10, 6: 78, 7: 8, 8: 16, 9: 2, 10: 2},          # H, W, kh, kw, sh, sw
    "maa_op_unfold": {3: 10, 4: 78, 5: 8, 6: 16, 7: 2, 8: 2},
    "maa_op_fold": {4: 10, 5: 78, 6: 8, 7: 16, 8: 2, 9: 2},
    "maa_ddim_stochastic_encode": {7: 10},                                             # n_tab
    "maa_ddpm_update": {8: 10},
    "maa_op_linear": {5: 32, 6: 0, 9: 0},                                              # N, geglu, c_split
    "maa_op_conv": {13: 0, 20: 0},                                                     # upsample2, c_split
    "maa_op_groupnorm_ex": {1: 32, 2: 32, 3: NULL, 4: 0, 5: 0, 8: 1, 14: 0, 15: NULL},          # one source of 32 channels, one group
    "maa_op_layernorm_ex": {2: 32},
    "maa_op_split32": {2: 32},
    "maa_op_attention_ex": {1: 8, 2: 8, 4: 8, 5: 8, 7: 8, 8: 8, 11: 8, 16: 8},         # pitches and head strides of one head of 8
    "maa_op_attention_masked": {1: 8, 2: 8, 4: 8, 5: 8, 7: 8, 8: 8, 11: 8, 16: 8},
    "maa_op_conv_transpose1d": {7: 4, 8: 2},                                           # k, stride
    "maa_op_mrf_pair": {6: 3, 12: 3},                                                  # k1, k2
    "maa_op_bench_conv": {5: 9},                                                       # taps
    "maa_resampler_create": {0: 2, 1: 1, 2: 3, 3: 8},
    "maa_calib": {0: 0}, "maa_ctx_set_precision": {0: 1}, "maa_ctx_set_cfg_split": {0: 1}, "maa_ctx_set_concurrency": {0: 1},
}
ENTRIES = sorted(set(L.SIGNATURES) - set(EXCEPTIONS))


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import build
    build.build(verbose=False)
    return L.load()


def _is_pointer(t):
    return t is C.c_void_p or hasattr(t, "_type_") and not isinstance(t._type_, str)


def _well_formed(name, configs):
    args = []
    over = WELL_FORMED.get(name, {})
    for i, t in enumerate(L.SIGNATURES[name][1:]):
        if i in over:
            args.append(None if over[i] is NULL else over[i])
        elif t is C.c_void_p:
            args.append(_base + 256 * i)          # distinct addresses: some entries refuse aliased buffers
        elif t is C.POINTER(C.c_float):
            args.append(C.cast(_base + 256 * i, t))
        elif t is C.POINTER(C.c_void_p):
            args.append(C.byref(C.c_void_p()))
        elif _is_pointer(t):
            args.append(configs[t._type_] if t._type_ in configs else C.byref(t._type_()))
        else:
            args.append(1)
    return args


def test_the_exceptions_are_entries_and_few():
    assert set(EXCEPTIONS) <= set(L.SIGNATURES) and len(ENTRIES) >= 65
    for name, reason in EXCEPTIONS.items():
        n = len(L.SIGNATURES[name])
        assert n == 1 or name in ("maa_ctx_create", "maa_prof_begin"), (name, reason)


@pytest.mark.parametrize("name", ENTRIES)
def test_a_malformed_call_is_refused_by_an_argument_check(lib, name):
    fn = getattr(lib, name)
    zeros = [None if _is_pointer(t) else 0 for t in L.SIGNATURES[name][1:]]
    if name in MALFORMED:
        zeros = list(MALFORMED[name])
    assert fn(None, *zeros) < 0
    assert len(lib.maa_last_error()) > 0 and b"null context" not in lib.maa_last_error(), lib.maa_last_error()


@pytest.mark.parametrize("kind", sorted(L.TTS_KINDS))
def test_every_kind_of_op_tts_rows_checks_before_the_context(lib, kind):
    """maa_op_tts_rows is ten launches behind one entry: the rule holds for each of them."""
    assert sorted(TTS_MALFORMED) == sorted(L.TTS_KINDS) == sorted(_tts_rows())
    good = _tts_rows()[kind]
    assert lib.maa_op_tts_rows(None, _struct(L.maa_tts_rows_args, **good)) < 0
    assert b"null context" in lib.maa_last_error(), lib.maa_last_error()
    assert lib.maa_op_tts_rows(None, _struct(L.maa_tts_rows_args, **dict(good, **TTS_MALFORMED[kind]))) < 0
    assert len(lib.maa_last_error()) > 0 and b"null context" not in lib.maa_last_error(), lib.maa_last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_a_well_formed_call_reaches_the_missing_context(lib, name):
    fn = getattr(lib, name)
    assert fn(None, *_well_formed(name, _configs())) < 0
    assert b"null context" in lib.maa_last_error(), lib.maa_last_error()
