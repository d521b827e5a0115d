"""Shape source of truth for the Make-An-Audio hot path, as plain dicts.

The reference keeps these in OmegaConf YAMLs (omegaconf is not available here):
  * T2A      text_to_audio/Make_An_Audio/configs/text_to_audio/txt2audio_args.yaml:1-78
  * I2A      text_to_audio/Make_An_Audio/configs/img_to_audio/img2audio_args.yaml:1-77
  * Inpaint  text_to_audio/Make_An_Audio/configs/inpaint/txt2audio_args.yaml:1-68
  * HiFi-GAN text_to_audio/Make_An_Audio/vocoder/logs/hifi_0127/args.yml:1-47,
             NeuralSeq/egs/egs_bases/tts/vocoder/hifigan.yaml:3-10 (uic 512),
             NeuralSeq/configs/tts/hifigan.yaml:3-10 (uic 128)
"""
from copy import deepcopy

# ---------------------------------------------------------------- UNet variants
UNET_T2A = dict(
    variant="t2a",
    in_channels=4, out_channels=4, model_channels=320,
    attention_resolutions=(1, 2), num_res_blocks=2, channel_mult=(1, 2),
    num_heads=8, num_head_channels=-1,
    use_spatial_transformer=True, transformer_depth=1, context_dim=1024,
    legacy=False, resblock_updown=False,
    add_context_to_emb=False,          # custom_openaimodel.py:352-354 (I2A only)
)

UNET_I2A = dict(
    variant="i2a",
    in_channels=4, out_channels=4, model_channels=256,
    attention_resolutions=(1, 2), num_res_blocks=2, channel_mult=(1, 2),
    num_heads=-1, num_head_channels=32,
    use_spatial_transformer=True, transformer_depth=1, context_dim=1024,
    legacy=True, resblock_updown=False,
    add_context_to_emb=True,
)

UNET_INPAINT = dict(
    variant="inpaint",
    in_channels=9, out_channels=4, model_channels=320,
    attention_resolutions=(1, 2), num_res_blocks=2, channel_mult=(1, 2),
    num_heads=8, num_head_channels=-1,
    use_spatial_transformer=False, transformer_depth=1, context_dim=None,
    legacy=True, resblock_updown=True,
    add_context_to_emb=False,
)

# ---------------------------------------------------------------- VAE (AutoencoderKL ddconfig)
VAE_DDCONFIG = dict(
    double_z=True, z_channels=4, resolution=848, in_channels=1, out_ch=1,
    ch=128, ch_mult=(1, 2, 2, 4), num_res_blocks=2, attn_resolutions=(106, 212),
    embed_dim=4,
)

# ---------------------------------------------------------------- diffusion schedules
LDM_T2A = dict(
    unet=UNET_T2A, vae=VAE_DDCONFIG, timesteps=1000,
    linear_start=0.00085, linear_end=0.0120,
    conditioning_key="crossattn", latent_shape=(4, 10, 78), scale_factor=1.0,
    sample_rate=16000, hop=256, log_every_t=200,
)
LDM_I2A = dict(
    unet=UNET_I2A, vae=VAE_DDCONFIG, timesteps=1000,
    linear_start=0.00085, linear_end=0.0120,
    conditioning_key="crossattn", latent_shape=(4, 10, 78), scale_factor=1.0,
    sample_rate=16000, hop=256, log_every_t=200,
)
LDM_INPAINT = dict(
    unet=UNET_INPAINT, vae=VAE_DDCONFIG, timesteps=1000,
    linear_start=0.0015, linear_end=0.0205,
    conditioning_key="concat", latent_shape=(4, 10, 106), scale_factor=1.0,
    sample_rate=16000, hop=256, log_every_t=100,
)

# ---------------------------------------------------------------- vocoders
HIFIGAN_16K = dict(           # MAA/vocoder/logs/hifi_0127/args.yml
    kind="hifigan", num_mels=80, upsample_initial_channel=512,
    upsample_rates=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
    resblock="1", resblock_kernel_sizes=(3, 7, 11),
    resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 5)),
    sampling_rate=16000,
)
HIFIGAN_NS_512 = dict(HIFIGAN_16K, sampling_rate=22050)                    # egs_bases/tts/vocoder/hifigan.yaml
HIFIGAN_NS_128 = dict(HIFIGAN_16K, sampling_rate=22050, upsample_initial_channel=128)  # configs/tts/hifigan.yaml

# The generators' other residual block (`resblock: "2"`: ResBlock2, hifigan.py:70-91 / modules.py:62-83; AMPBlock2,
# bigvgan/models.py:90-132): no shipped config selects it -- these are HiFi-GAN's published V3 shapes (hop 256), and
# the same with BigVGAN's plain `snake` activation (activations.py:8-59), which BIGVGAN_16K does not exercise either.
HIFIGAN_RB2 = dict(HIFIGAN_16K, upsample_initial_channel=256, upsample_rates=(8, 8, 4), upsample_kernel_sizes=(16, 16, 8),
                   resblock="2", resblock_kernel_sizes=(3, 5, 7), resblock_dilation_sizes=((1, 2), (2, 6), (3, 12)))
BIGVGAN_RB2 = dict(HIFIGAN_RB2, kind="bigvgan", activation="snake", snake_logscale=False)

# NSF (f0-conditioned) generator of the singing tools: checkpoints/0109_hifigan_bigpopcs_hop128 is not shipped, so the
# rates are the hop-128 / 24 kHz factorisation assumed here (egs_bases/svs/popcs_ds_beta6.yaml:6-7,54-55,70); used by the
# oracle groundwork for SURVEY 8f/N1 only.
HIFIGAN_NSF_24K = dict(HIFIGAN_16K, sampling_rate=24000, upsample_rates=(8, 4, 2, 2), upsample_kernel_sizes=(16, 8, 4, 4),
                       use_pitch_embed=True)

# DiffSinger denoiser + PLMS loop of the T2S tool (egs_bases/svs/base.yaml:3-5, midi/e2e/opencpop/ds1000.yaml:22-36;
# checkpoints/0831_opencpop_ds1000): oracle groundwork for SURVEY 8f/N2 only.
DIFFSINGER_DS1000 = dict(in_dims=80, hidden_size=256, residual_layers=20, residual_channels=256, dilation_cycle_length=4,
                         timesteps=1000, K_step=1000, max_beta=0.02, pndm_speedup=10, schedule_type="linear")

# The configurations without pndm_speedup: the reference samples them with the ancestral chain, K_step p_sample steps
# (shallow_diffusion_tts.py:269-271).  hidden_size 256 is the FastSpeech2 default they inherit; residual_layers / residual_channels /
# dilation_cycle_length / timesteps come from egs_bases/svs/base.yaml:3-6.  spec_min / spec_max (80 values, in the same files)
# belong to the checkpoint and are passed to GaussianDiffusion by the caller.
# egs_bases/svs/popcs_ds_beta6.yaml:63-68 (DiffSinger on PopCS, shallow diffusion from the fs2 mel at t = 50)
DIFFSINGER_POPCS_BETA6 = dict(in_dims=80, hidden_size=256, residual_layers=20, residual_channels=256, dilation_cycle_length=1,
                              timesteps=100, K_step=51, max_beta=0.06, schedule_type="linear")
# egs_bases/svs/lj_ds_beta6.yaml:36-41 (DiffSpeech on LJSpeech)
DIFFSPEECH_LJ_BETA6 = dict(DIFFSINGER_POPCS_BETA6, K_step=71)
# egs_bases/svs/midi/e2e/opencpop/ds100_adj_rel.yaml:22-32 and midi/e2e/popcs/ds100_adj_rel.yaml over popcs_ds_beta6.yaml: the
# whole chain from Gaussian noise
DIFFSINGER_DS100_ADJ_REL = dict(DIFFSINGER_POPCS_BETA6, dilation_cycle_length=4, K_step=100, gaussian_start=True)

# PitchExtractor of the e2e singing configurations (pe_enable: true in midi/e2e/opencpop/ds1000.yaml, ds100_adj_rel.yaml,
# ds1000-10dil.yaml, midi/e2e/popcs/ds100_adj_rel.yaml): egs_bases/svs/midi/pe.yaml (pitch_type frame, predictor_hidden -1,
# conv_layers 2 = PitchExtractor's default) over the FastSpeech2 defaults of egs_bases/tts/fs2.yaml and base.yaml (hidden_size
# 256, predictor_kernel 5, ffn_padding SAME, use_uv true, pitch_norm log).  f0_mean / f0_std are read with pitch_norm 'standard'
# only.  checkpoints/0102_xiaoma_pe is not shipped.
PITCH_EXTRACTOR = dict(n_mel_bins=80, hidden_size=256, predictor_hidden=-1, predictor_kernel=5, ffn_padding="SAME", conv_layers=2,
                       pitch_type="frame", use_uv=True, pitch_norm="log", f0_mean=0.0, f0_std=1.0)

# FastSpeech2MIDI of the e2e singing configurations (midi/e2e/opencpop/ds1000.yaml, ds1000-10dil.yaml, ds100_adj_rel.yaml,
# midi/e2e/popcs/ds100_adj_rel.yaml): the hparams modules/diffsinger_midi/fs2.py and modules/fastspeech/fs2.py read, with the values
# those files resolve to over egs_bases/tts/fs2.yaml and base.yaml (rel_pos true in the e2e files; use_pitch_embed false there: the
# pitch comes from the extractor after the diffusion).  vocab_size = len(phone_encoder) of the checkpoint's dictionary -- a
# placeholder here, the dictionary is not shipped; index 0 is the padding token.
FASTSPEECH2_MIDI = dict(vocab_size=64, hidden_size=256, enc_layers=4, dec_layers=4, num_heads=2, enc_ffn_kernel_size=9,
                        dec_ffn_kernel_size=9, dur_predictor_layers=5, dur_predictor_kernel=3, predictor_hidden=-1,
                        audio_num_mel_bins=80, ffn_padding="SAME", ffn_act="gelu", dur_loss="mse", rel_pos=True, use_pos_embed=True,
                        encoder_type="fft", decoder_type="fft", use_pitch_embed=False, use_energy_embed=False, use_spk_id=False,
                        use_spk_embed=False, use_bert=False)
# FastSpeech2MIDI of the cascade singing configuration (inference/svs/ds_cascade.py): egs_bases/svs/midi/cascade/opencs/ds60_rel.yaml
# with its fs2 in aux_rel.yaml, over egs_bases/tts/fs2.yaml and egs_bases/singing/base.yaml: use_pitch_embed true, the frame-level
# pitch predictor (5 layers, kernel 5) with a voicing logit, log2 f0 (f0_mean / f0_std are read with pitch_norm 'standard' only).
# popcs_ds_beta6.yaml and lj_ds_beta6.yaml resolve to the same pitch hparams over the plain (non-MIDI) encoder, which is not built.
FASTSPEECH2_MIDI_CASCADE = dict(FASTSPEECH2_MIDI, use_pitch_embed=True, pitch_type="frame", use_uv=True, pitch_norm="log",
                                pitch_ar=False, predictor_layers=5, predictor_kernel=5, f0_mean=0.0, f0_std=1.0)

# The plain FastSpeech2 (modules/fastspeech/fs2.py) of the TTS configurations: egs_bases/tts/fs2.yaml over egs_bases/tts/base.yaml
# (4 + 4 layers, 2 heads, 9-tap FFNs, dur_predictor 2 layers / kernel 3, predictor 2 layers / kernel 5, the frame-level pitch branch
# with a voicing logit, pitch_norm standard; no rel_pos: sinusoid positions by token count; use_energy_embed false).  vocab_size is
# a placeholder as above; f0_mean / f0_std are the data set's statistics, written into hparams by its binarizer -- placeholders.
# It is also the `fs2` of both *_ds_beta6 chains (DIFFSPEECH_LJ_BETA6, DIFFSINGER_POPCS_BETA6).
FASTSPEECH2 = dict(vocab_size=64, hidden_size=256, enc_layers=4, dec_layers=4, num_heads=2, enc_ffn_kernel_size=9,
                   dec_ffn_kernel_size=9, dur_predictor_layers=2, dur_predictor_kernel=3, predictor_hidden=-1, predictor_layers=2,
                   predictor_kernel=5, audio_num_mel_bins=80, ffn_padding="SAME", ffn_act="gelu", dur_loss="mse", rel_pos=False,
                   use_pos_embed=True, encoder_type="fft", decoder_type="fft", use_pitch_embed=True, pitch_type="frame", use_uv=True,
                   pitch_norm="standard", pitch_ar=False, f0_mean=220.0, f0_std=60.0, use_energy_embed=False, use_spk_id=False,
                   use_split_spk_id=False, use_spk_embed=False, num_spk=1, use_bert=False)
# egs/datasets/audio/libritts/fs2.yaml (use_spk_id true, num_spk 2320; vctk/fs2.yaml: 400)
FASTSPEECH2_LIBRITTS = dict(FASTSPEECH2, use_spk_id=True, num_spk=2320)

# The Glow post-net GenerSpeech runs in reverse over its decoder's mel (modules/GenerSpeech/model/generspeech.py:57-72, 233-260):
# modules/GenerSpeech/config/generspeech.yaml:83-92 (post_glow_hidden 128, post_glow_kernel_size 3, post_glow_n_blocks 8,
# post_glow_n_block_layers 3, share_wn_layers 4, sigmoid_scale false, post_share_cond_layers false, use_txt_cond true, noise_scale
# 0.8) over hidden_size 256.  The conditioning is [mel_out 80 | decoder_inp 256 | spk, emo, ref_prosody 3 x 256] = 1104 channels.
GENERSPEECH_POST_GLOW = dict(in_channels=80, hidden_channels=128, kernel_size=3, dilation_rate=1, n_blocks=8, n_layers=3, n_split=4,
                             n_sqz=2, gin_channels=80 + 256 + 3 * 256, share_cond_layers=False, share_wn_layers=4,
                             sigmoid_scale=False, inv_conv_type="near", p_dropout=0.0, hidden_size=256, use_txt_cond=True,
                             n_cond_vectors=3, noise_scale=0.8)
# PortaSpeech's post-net, egs_bases/tts/ps_flow.yaml:7-18 (post_glow_hidden 192, 12 blocks, 3 layers, share_wn_layers 4, noise_scale
# 0.8) over hidden_size 192: the conditioning is [mel_out 80 | decoder_inp 192], no per-utterance vectors.
PORTASPEECH_POST_GLOW = dict(GENERSPEECH_POST_GLOW, hidden_channels=192, n_blocks=12, gin_channels=80 + 192, hidden_size=192,
                             n_cond_vectors=0)

# BigVGAN's args.yml (vocoder/logs/bigv16k53w) does not ship with the reference
# (SURVEY.md section 0.3); these are the generator defaults it is exercised with here.
BIGVGAN_16K = dict(
    HIFIGAN_16K, kind="bigvgan", activation="snakebeta", snake_logscale=True,
)

# ---------------------------------------------------------------- conditioning encoders
# CLAP text branch: transformers' bert-base-uncased + Projection 768 -> 1024 (encoders/CLAP/config.yml, CLAP/clap.py:8-45);
# FrozenCLAPEmbedder pads / truncates to 77 tokens (encoders/modules.py:175,204-206)
CLAP_TEXT = dict(kind="text", layers=12, width=768, heads=12, mlp_dim=3072, d_proj=1024, vocab=30522, max_positions=512,
                 type_vocab=2, ln_eps=1e-12, max_length=77)
# OpenCLIP ViT-H-14 image tower (open_clip model config "ViT-H-14": width 1280, 32 layers, head width 80, mlp ratio 4,
# patch 14, image 224, embed_dim 1024), as FrozenGlobalNormOpenCLIPEmbedder builds it (encoders/modules.py:319-321)
OPENCLIP_VITH14_IMAGE = dict(kind="image", layers=32, width=1280, heads=16, mlp_dim=5120, d_proj=1024, patch=14, image=224,
                             ln_eps=1e-5)
# OpenCLIP ViT-H-14 text tower (open_clip model config "ViT-H-14": context 77, vocab 49408, width 1024, 16 heads,
# 24 layers, embed_dim 1024): FrozenGlobalNormOpenCLIPEmbedder.forward -- I2A's unconditional prompt (audio-chatgpt.py:238)
OPENCLIP_VITH14_TEXT = dict(kind="clip_text", layers=24, width=1024, heads=16, mlp_dim=4096, d_proj=1024, vocab=49408,
                            max_positions=77, ln_eps=1e-5, sot=49406, eot=49407)
# CLAP audio branch of the best-of-n scorer (wav_evaluation/models/CLAPWrapper.py, useful_ckpts/CLAP/config.yml): Cnn14 on
# a 64-bin log-mel at 44.1 kHz (window 1024, hop 320), 2048-d embedding -> Projection -> 1024.  `frames` is only the
# length of the golden test case (690 frames = 5 s); the scorer's own clips are `duration` * the INPUT sample rate long.
CLAP_AUDIO_CNN14 = dict(mel_bins=64, channels=(64, 128, 256, 512, 1024, 2048), out_emb=2048, d_proj=1024, classes_num=527,
                        sample_rate=44100, window_size=1024, hop_size=320, fmin=50, fmax=14000, frames=690)


# The whole scorer as T2A.select_best_audio builds it (audio-chatgpt.py:185-199; useful_ckpts/CLAP/config.yml):
# text side = the same BERT + Projection architecture as CLAP_TEXT, padded to text_len with an attention mask
CLAP_SCORER = dict(text=dict(CLAP_TEXT, max_length=100), audio=CLAP_AUDIO_CNN14, sampling_rate=44100, duration=9, text_len=100,
                   window_size=1024, hop_size=320, mel_bins=64, fmin=50, fmax=14000, amin=1e-10, ref=1.0,
                   resample=dict(lowpass_filter_width=6, rolloff=0.99))


def small(cfg, **over):
    """A reduced copy of a config for quick tests."""
    c = deepcopy(cfg)
    c.update(over)
    return c


def hop_size(voc_cfg):
    h = 1
    for u in voc_cfg["upsample_rates"]:
        h *= u
    return h
