"""ctypes binding of libaudiogpt_mi355x.so (include/maa.h).  This is the binding a maintainer of the
reference would add; PyTorch is only used for device memory and the current stream.

There is no CPU fallback: if the shared object is missing or fails to load, importing the backend raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# AUDIOGPT_AMD_LIB: another build of the same library (same-box A/B of two builds; never a different implementation)
LIB_PATH = os.environ.get("AUDIOGPT_AMD_LIB") or os.path.join(_HERE, "libaudiogpt_mi355x.so")


class MaaError(RuntimeError):
    pass


class maa_tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("ndim", C.c_int), ("shape", C.c_int64 * 6)]


class maa_prof_row(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


class maa_unet_config(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("model_channels", C.c_int),
                ("num_res_blocks", C.c_int),
                ("n_channel_mult", C.c_int), ("channel_mult", C.c_int * 8),
                ("n_attention_resolutions", C.c_int), ("attention_resolutions", C.c_int * 8),
                ("num_heads", C.c_int), ("num_head_channels", C.c_int),
                ("use_spatial_transformer", C.c_int), ("transformer_depth", C.c_int), ("context_dim", C.c_int),
                ("legacy", C.c_int), ("resblock_updown", C.c_int), ("add_context_to_emb", C.c_int)]


class maa_ddim_args(C.Structure):
    _fields_ = [("S", C.c_int), ("B", C.c_int), ("C", C.c_int), ("H", C.c_int), ("W", C.c_int),
                ("scale", C.c_float),
                ("d_cond", C.c_void_p), ("d_uncond", C.c_void_p), ("L", C.c_int),
                ("d_concat", C.c_void_p), ("Cc", C.c_int),
                ("h_timesteps", C.POINTER(C.c_int32)), ("h_alphas", C.POINTER(C.c_float)),
                ("h_alphas_prev", C.POINTER(C.c_float)), ("use_graph", C.c_int),
                ("d_mask", C.c_void_p), ("d_x0", C.c_void_p), ("d_noise_q", C.c_void_p),
                ("h_sqrt_ac", C.POINTER(C.c_float)), ("h_sqrt_1mac", C.POINTER(C.c_float)),
                ("h_sigmas", C.POINTER(C.c_float)), ("d_noise_p", C.c_void_p), ("temperature", C.c_float),
                ("log_every_t", C.c_int), ("n_log", C.c_int), ("d_log_x", C.c_void_p), ("d_log_x0", C.c_void_p),
                ("split_kh", C.c_int), ("split_kw", C.c_int), ("split_sh", C.c_int), ("split_sw", C.c_int),
                ("h_split_weight", C.POINTER(C.c_float))]


class maa_ddpm_args(C.Structure):
    _fields_ = [("loop", maa_ddim_args), ("start", C.c_int), ("n", C.c_int), ("clip_denoised", C.c_int),
                ("h_sqrt_recip_ac", C.POINTER(C.c_float)), ("h_sqrt_recipm1_ac", C.POINTER(C.c_float)),
                ("h_coef1", C.POINTER(C.c_float)), ("h_coef2", C.POINTER(C.c_float)), ("h_logvar", C.POINTER(C.c_float)),
                ("h_sqrt_ac", C.POINTER(C.c_float)), ("h_sqrt_1mac", C.POINTER(C.c_float)),
                ("h_temperature", C.POINTER(C.c_float))]


class maa_vae_config(C.Structure):
    _fields_ = [("ch", C.c_int), ("out_ch", C.c_int), ("in_channels", C.c_int), ("z_channels", C.c_int),
                ("embed_dim", C.c_int), ("resolution", C.c_int), ("num_res_blocks", C.c_int), ("double_z", C.c_int),
                ("n_ch_mult", C.c_int), ("ch_mult", C.c_int * 8),
                ("n_attn_resolutions", C.c_int), ("attn_resolutions", C.c_int * 8)]


class maa_vocoder_config(C.Structure):
    _fields_ = [("kind", C.c_int), ("num_mels", C.c_int), ("upsample_initial_channel", C.c_int),
                ("n_upsamples", C.c_int), ("upsample_rates", C.c_int * 8), ("upsample_kernel_sizes", C.c_int * 8),
                ("n_kernels", C.c_int), ("resblock_kernel_sizes", C.c_int * 8),
                ("n_dilations", C.c_int), ("resblock_dilation_sizes", (C.c_int * 8) * 8),
                ("snake_beta", C.c_int), ("snake_logscale", C.c_int),
                ("use_pitch_embed", C.c_int), ("sampling_rate", C.c_int), ("harmonic_num", C.c_int),
                ("resblock", C.c_int)]


class maa_diffnet_config(C.Structure):
    _fields_ = [("in_dims", C.c_int), ("hidden_size", C.c_int), ("residual_layers", C.c_int),
                ("residual_channels", C.c_int), ("dilation_cycle_length", C.c_int)]


class maa_pitch_extractor_config(C.Structure):
    _fields_ = [("n_mel_bins", C.c_int), ("hidden_size", C.c_int), ("predictor_hidden", C.c_int), ("predictor_kernel", C.c_int),
                ("conv_layers", C.c_int), ("ffn_padding_same", C.c_int), ("use_uv", C.c_int), ("pitch_norm", C.c_int),
                ("f0_mean", C.c_float), ("f0_std", C.c_float)]


class maa_glow_config(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "in_channels", "hidden_channels", "kernel_size", "dilation_rate", "n_blocks", "n_layers", "n_split", "n_sqz",
        "gin_channels", "share_cond_layers", "share_wn_layers", "sigmoid_scale")]


class maa_fs2_config(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "vocab_size", "hidden_size", "enc_layers", "dec_layers", "num_heads", "enc_ffn_kernel_size", "dec_ffn_kernel_size",
        "dur_predictor_layers", "dur_predictor_kernel", "predictor_hidden", "audio_num_mel_bins",
        "ffn_padding_same", "ffn_act_gelu", "dur_loss_mse", "rel_pos", "use_pos_embed", "encoder_fft", "decoder_fft",
        "use_pitch_embed", "use_energy_embed", "use_spk_id", "use_spk_embed", "use_bert",
        "plain", "num_spk", "use_split_spk_id", "predictor_layers", "predictor_kernel")]


class maa_fs2_pitch_config(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "hidden_size", "predictor_hidden", "predictor_layers", "predictor_kernel", "ffn_padding_same", "pitch_type_frame",
        "pitch_ar", "use_uv", "pitch_norm")] + [("f0_mean", C.c_float), ("f0_std", C.c_float)]


class maa_encoder_config(C.Structure):
    _fields_ = [("kind", C.c_int), ("layers", C.c_int), ("width", C.c_int), ("heads", C.c_int), ("mlp_dim", C.c_int),
                ("d_proj", C.c_int), ("vocab", C.c_int), ("max_positions", C.c_int), ("patch", C.c_int),
                ("image", C.c_int), ("ln_eps", C.c_float)]


class maa_clap_audio_config(C.Structure):
    _fields_ = [("mel_bins", C.c_int), ("n_blocks", C.c_int), ("channels", C.c_int * 8), ("out_emb", C.c_int),
                ("d_proj", C.c_int), ("bn_eps", C.c_float)]


class maa_spectral_config(C.Structure):
    _fields_ = [("n_fft", C.c_int), ("hop", C.c_int), ("n_freq", C.c_int), ("n_mels", C.c_int), ("pad_mode", C.c_int),
                ("power", C.c_int), ("log_kind", C.c_int), ("amin", C.c_float), ("ref", C.c_float), ("out_layout", C.c_int)]


class maa_plms_args(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("K_step", C.c_int), ("interval", C.c_int), ("timesteps", C.c_int),
                ("d_cond", C.c_void_p), ("h_alphas_cumprod", C.POINTER(C.c_float)), ("use_graph", C.c_int)]


class maa_ds_ddpm_args(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("start", C.c_int), ("n", C.c_int), ("timesteps", C.c_int),
                ("clip_denoised", C.c_int), ("use_graph", C.c_int),
                ("d_cond", C.c_void_p), ("d_noise", C.c_void_p),
                ("h_sqrt_recip_ac", C.POINTER(C.c_float)), ("h_sqrt_recipm1_ac", C.POINTER(C.c_float)),
                ("h_coef1", C.POINTER(C.c_float)), ("h_coef2", C.POINTER(C.c_float)), ("h_sigma", C.POINTER(C.c_float))]


class maa_igemm_ex_args(C.Structure):
    _fields_ = [("d_x1", C.c_void_p), ("ld1", C.c_int), ("C1", C.c_int), ("d_x2", C.c_void_p), ("ld2", C.c_int), ("C2", C.c_int),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Ho", C.c_int), ("Wo", C.c_int),
                ("h_w", C.POINTER(C.c_float)), ("h_bias", C.POINTER(C.c_float)), ("Cout", C.c_int), ("KH", C.c_int), ("KW", C.c_int),
                ("stride", C.c_int), ("pad_w", C.c_int), ("pad_h", C.c_int), ("dil", C.c_int), ("up", C.c_int),
                ("a_leaky", C.c_float), ("presplit", C.c_int),
                ("alpha", C.c_float), ("d_rowadd", C.c_void_p), ("ld_rowadd", C.c_int), ("d_res", C.c_void_p), ("ldr", C.c_int),
                ("act", C.c_int), ("act_slope", C.c_float), ("out_scale", C.c_float),
                ("accumulate", C.c_int), ("geglu", C.c_int), ("c_split", C.c_int),
                ("d_c", C.c_void_p), ("ldc", C.c_int), ("d_c2", C.c_void_p), ("ldc2", C.c_int), ("c2_slope", C.c_float)]


class maa_seq_rows_args(C.Structure):
    _fields_ = [("kind", C.c_int), ("rows", C.c_int), ("B", C.c_int), ("T", C.c_int), ("C", C.c_int),
                ("d_x", C.c_void_p), ("d_res", C.c_void_p), ("d_mask", C.c_void_p),
                ("h_scale", C.POINTER(C.c_float)), ("h_shift", C.POINTER(C.c_float)), ("h_gamma", C.POINTER(C.c_float)),
                ("h_beta", C.POINTER(C.c_float)), ("h_w", C.POINTER(C.c_float)), ("h_bias", C.POINTER(C.c_float)),
                ("groups", C.c_int), ("eps", C.c_float), ("table_rows", C.c_int), ("alpha", C.c_float),
                ("n_out", C.c_int), ("pitch_norm", C.c_int), ("f0_mean", C.c_float), ("f0_std", C.c_float), ("use_uv", C.c_int),
                ("d_out", C.c_void_p), ("d_out2", C.c_void_p), ("d_pos", C.c_void_p), ("d_dur", C.c_void_p)]


SEQ_KINDS = {"frame_mask": 0, "affine_mask": 1, "gn_relu_res": 2, "pos_add": 3, "head": 4}      # MAA_SEQ_* of include/maa.h


class maa_tts_rows_args(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "kind", "rows", "B", "T", "C", "H", "first", "last", "sigmoid_scale", "rel", "split", "vocab", "pe_rows", "n_rows")] + [
        ("eps", C.c_float), ("alpha", C.c_float)] + [(k, C.c_void_p) for k in (
            "d_x", "d_y", "d_mask", "d_spk", "d_energy", "d_tok", "d_mel2ph", "d_ids")] + [(k, C.POINTER(C.c_float)) for k in (
                "h_gamma", "h_beta", "h_w", "h_bias", "h_table", "h_t1", "h_t2", "h_pe", "h_winv", "h_an_bias", "h_an_einv")] + [
        (k, C.c_void_p) for k in ("d_out", "d_out2", "d_out3", "d_rowld", "d_h_cpl", "d_h_inv", "d_h_act", "d_energy_pred", "d_bin")]


# MAA_TTS_* of include/maa.h
TTS_KINDS = {"glow_squeeze": 0, "glow_gate": 1, "glow_wn_residual": 2, "glow_block_tail": 3, "glow_logdet": 4, "fs2_embed_plain": 5,
             "fs2_add_speaker": 6, "fs2_speaker_gather": 7, "fs2_energy_tail": 8, "fs2_tgt_mask": 9}


class maa_sampler_step_args(C.Structure):
    _fields_ = [("kind", C.c_int), ("B", C.c_int), ("nB", C.c_int), ("S", C.c_int),
                ("n", C.c_int64), ("per", C.c_int64), ("per_in", C.c_int64),
                ("scale", C.c_float), ("temperature", C.c_float),
                ("start", C.c_int), ("clip", C.c_int), ("mode", C.c_int), ("interval", C.c_int), ("timesteps", C.c_int),
                ("n_steps", C.c_int), ("emb_w", C.c_int), ("n_t", C.c_int)] + [(k, C.c_void_p) for k in (
        "d_x", "d_concat", "d_xin", "d_eps_u", "d_eps_c", "d_e_prev", "d_coef", "d_tab_t", "d_tab", "d_step", "d_st", "d_cur_t",
        "d_emb_tab", "d_cur_emb", "d_mask", "d_x0", "d_noise_q", "d_noise_p", "d_ring", "d_e_keep", "d_x_out", "d_log_x",
        "d_log_x0")]


# MAA_STEP_* of include/maa.h
STEP_KINDS = {"ddim_prepare": 0, "ddim": 1, "plms": 2, "plms_euler_mid": 3, "plms_euler_final": 4, "ddpm": 5, "ds_plms": 6,
              "ds_advance": 7, "ds_ddpm": 8}


class maa_front_rows_args(C.Structure):
    _fields_ = [(k, C.c_int) for k in (
        "kind", "B", "rows", "n", "T", "F", "C", "left", "total", "ldo", "mode", "nf", "ldy", "ldm", "power2",
        "frames", "n_mels", "ldmel", "log_kind", "layout")] + [
        ("amin", C.c_float), ("ref_db", C.c_float), ("d_x", C.c_void_p), ("h_scale", C.POINTER(C.c_float)),
        ("h_shift", C.POINTER(C.c_float)), ("d_out", C.c_void_p)]


FRONT_KINDS = {"pad": 0, "power": 1, "logmel": 2, "affine": 3, "pool": 4}      # MAA_FRONT_* of include/maa.h

# The one list of the library's entries: name -> argument types (every entry returns an int status).  load() applies it and
# EXPORTS is derived from it; a new entry of include/maa.h is added here and nowhere else.
vp, ci, cf, fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_float)
SIGNATURES = {
    "maa_ctx_create": [ci, vp, C.POINTER(vp)],
    "maa_ctx_destroy": [vp],
    "maa_ctx_synchronize": [vp],
    "maa_ctx_set_stream": [vp, vp],
    "maa_ctx_workspace_bytes": [vp, C.POINTER(C.c_size_t)],
    "maa_ctx_set_precision": [vp, ci],
    "maa_ctx_set_cfg_split": [vp, ci],
    "maa_ctx_set_concurrency": [vp, ci],
    "maa_ctx_reload_tuning": [vp],
    "maa_prof_begin": [vp, ci],
    "maa_prof_end": [vp, C.POINTER(maa_prof_row), ci, C.POINTER(ci)],
    "maa_unet_create": [vp, C.POINTER(maa_unet_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_unet_destroy": [vp],
    "maa_unet_set_context": [vp, vp, vp, ci, ci],
    "maa_unet_forward": [vp, vp, vp, vp, ci, ci, ci, vp],
    "maa_ddim_update": [vp, vp, vp, vp, cf, vp, C.c_int64, vp, vp],
    "maa_ddim_sample": [vp, vp, C.POINTER(maa_ddim_args), vp],
    "maa_ddim_stochastic_encode": [vp, vp, ci, cf, vp, vp, fp, fp, ci, vp, ci, ci, ci, ci, vp],
    "maa_ddim_decode": [vp, vp, C.POINTER(maa_ddim_args), ci, vp],
    "maa_ldm_plms_sample": [vp, vp, C.POINTER(maa_ddim_args), vp],
    "maa_ddpm_sample": [vp, vp, C.POINTER(maa_ddpm_args), vp],
    "maa_ddpm_update": [vp, vp, vp, vp, fp, fp, fp, fp, fp, ci, vp, cf, ci, ci, ci, ci, ci, vp, vp],
    "maa_vae_create": [vp, C.POINTER(maa_vae_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_vae_destroy": [vp],
    "maa_vae_decode": [vp, vp, vp, ci, ci, ci, cf, vp],
    "maa_vae_decode_spec": [vp, vp, vp, ci, ci, ci, cf, vp],
    "maa_vae_encode_moments": [vp, vp, vp, ci, ci, ci, vp],
    "maa_vocoder_create": [vp, C.POINTER(maa_vocoder_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_vocoder_destroy": [vp],
    "maa_vocoder_forward": [vp, vp, vp, ci, ci, vp],
    "maa_vocoder_forward_f0": [vp, vp, vp, vp, vp, vp, ci, ci, vp],
    "maa_diffnet_create": [vp, C.POINTER(maa_diffnet_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_diffnet_destroy": [vp],
    "maa_diffnet_forward": [vp, vp, vp, vp, vp, ci, ci, vp],
    "maa_plms_sample": [vp, vp, C.POINTER(maa_plms_args), vp],
    "maa_ds_ddpm_sample": [vp, vp, C.POINTER(maa_ds_ddpm_args), vp],
    "maa_ds_ddpm_update": [vp, vp, vp, vp, fp, fp, fp, fp, fp, ci, ci, ci, ci, ci, vp],
    "maa_pitch_extractor_create": [vp, C.POINTER(maa_pitch_extractor_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_pitch_extractor_destroy": [vp],
    "maa_pitch_extractor_forward": [vp, vp, vp, ci, ci, vp, vp, vp],
    "maa_glow_create": [vp, C.POINTER(maa_glow_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_glow_destroy": [vp],
    "maa_glow_reverse": [vp, vp, vp, vp, vp, ci, ci, vp, vp, vp],
    "maa_fs2_create": [vp, C.POINTER(maa_fs2_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_fs2_destroy": [vp],
    "maa_fs2_encode": [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp],
    "maa_fs2_encode_plain": [vp, vp, vp, vp, ci, ci, vp, vp, vp, vp],
    "maa_fs2_speaker": [vp, vp, vp, vp, ci, vp],
    "maa_fs2_add_speaker": [vp, vp, vp, vp, vp, ci, ci, vp],
    "maa_fs2_finish": [vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp],
    "maa_fs2_length_regulate": [vp, vp, vp, ci, ci, ci, vp],
    "maa_fs2_decode": [vp, vp, vp, vp, ci, ci, ci, vp, vp],
    "maa_fs2_run_decoder": [vp, vp, vp, vp, ci, ci, vp],
    "maa_fs2_pitch_create": [vp, C.POINTER(maa_fs2_pitch_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_fs2_pitch_destroy": [vp],
    "maa_fs2_pitch_forward": [vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp],
    "maa_fs2_pitch_forward_from": [vp, vp, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp],
    "maa_encoder_create": [vp, C.POINTER(maa_encoder_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_encoder_destroy": [vp],
    "maa_encoder_text": [vp, vp, vp, ci, ci, vp],
    "maa_encoder_image": [vp, vp, vp, ci, vp],
    "maa_encoder_text_cls": [vp, vp, vp, ci, ci, vp],
    "maa_clap_audio_create": [vp, C.POINTER(maa_clap_audio_config), C.POINTER(maa_tensor), ci, C.POINTER(vp)],
    "maa_clap_audio_destroy": [vp],
    "maa_clap_audio_embed": [vp, vp, vp, ci, ci, vp, vp],
    "maa_clap_similarity": [vp, vp, vp, ci, ci, ci, cf, vp],
    "maa_spectral_create": [vp, C.POINTER(maa_spectral_config), fp, fp, C.POINTER(vp)],
    "maa_spectral_destroy": [vp],
    "maa_spectral_forward": [vp, vp, vp, ci, ci, vp],
    "maa_resampler_create": [vp, ci, ci, ci, ci, fp, C.POINTER(vp)],
    "maa_resampler_destroy": [vp],
    "maa_resampler_forward": [vp, vp, vp, ci, ci, vp],
    "maa_op_linear": [vp, vp, ci, ci, fp, fp, ci, ci, vp, vp, ci],
    "maa_op_conv": [vp, vp, ci, ci, ci, ci, fp, fp, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, vp, vp, ci],
    "maa_op_groupnorm": [vp, vp, ci, ci, ci, fp, fp, cf, ci, vp],
    "maa_op_layernorm": [vp, vp, ci, ci, fp, fp, cf, vp],
    "maa_op_attention": [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, vp],
    "maa_op_attention_ex": [vp, vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, ci],
    "maa_op_attention_masked": [vp, vp, ci, ci, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, ci, cf, vp, ci, ci, ci, vp],
    "maa_op_conv_transpose1d": [vp, vp, ci, ci, ci, fp, fp, ci, ci, ci, cf, vp],
    "maa_op_snake_aa": [vp, vp, ci, ci, ci, fp, fp, ci, vp],
    "maa_op_bench_conv": [vp, ci, ci, ci, ci, ci, ci, ci, ci, C.POINTER(C.c_float)],
    "maa_calib": [vp, ci, C.POINTER(C.c_double)],
    "maa_op_mrf_pair": [vp, vp, ci, ci, ci, fp, fp, ci, ci, cf, fp, fp, ci, ci, cf, cf, ci, vp],
    "maa_op_groupnorm_ex": [vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, fp, fp, cf, ci, vp, ci, vp],
    "maa_op_igemm_ex": [vp, C.POINTER(maa_igemm_ex_args)],
    "maa_op_layernorm_ex": [vp, vp, ci, ci, fp, fp, cf, vp, ci],
    "maa_op_seq_rows": [vp, C.POINTER(maa_seq_rows_args)],
    "maa_op_tts_rows": [vp, C.POINTER(maa_tts_rows_args)],
    "maa_op_sampler_step": [vp, C.POINTER(maa_sampler_step_args)],
    "maa_op_front_rows": [vp, C.POINTER(maa_front_rows_args)],
    "maa_op_split32": [vp, vp, ci, ci, cf, ci, vp],
    "maa_unet_forward_split": [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, fp, vp],
    "maa_op_unfold": [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp],
    "maa_op_fold": [vp, vp, fp, ci, ci, ci, ci, ci, ci, ci, ci, vp],
}
del vp, ci, cf, fp

# every symbol include/maa.h declares: the two that return a string, then the table's
EXPORTS = ["maa_last_error", "maa_version"] + list(SIGNATURES)

_lib = None


def load():
    """Load the shared object (once).  Raises MaaError if it is missing: there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MaaError("%s not found -- run `python -m audiogpt_amd.build` (hipcc, gfx950)" % LIB_PATH)
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:
        raise MaaError("cannot load %s: %s" % (LIB_PATH, e))
    lib.maa_last_error.restype = C.c_char_p
    lib.maa_version.restype = C.c_char_p
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    _lib = lib
    return lib


def check(status):
    if status != 0:
        raise MaaError("libaudiogpt_mi355x: %s (status %d)" % (load().maa_last_error().decode(), status))


def host_f32(t):
    """A contiguous fp32 CPU tensor and its float* (keep the tensor alive while the pointer is used)."""
    t = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
    return t, C.cast(t.data_ptr(), C.POINTER(C.c_float))


def tensor_list(state_dict):
    """state_dict {name: tensor} -> (maa_tensor array, n, keepalive)."""
    items = list(state_dict.items())
    arr = (maa_tensor * len(items))()
    keep = []
    for i, (name, t) in enumerate(items):
        ht, ptr = host_f32(t)
        bname = name.encode()
        keep.append((ht, bname))
        arr[i].name = bname
        arr[i].data = ptr
        arr[i].ndim = ht.dim()
        for d, s in enumerate(ht.shape):
            arr[i].shape[d] = s
    return arr, len(items), keep


def dptr(t):
    """Device pointer of a contiguous fp32 CUDA(HIP) tensor."""
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())
