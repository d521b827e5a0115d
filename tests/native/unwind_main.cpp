// Constructor unwinding of the model executors (csrc/models.h): every class is constructed from a valid configuration and an
// empty state dict (Spectral and Resampler, which take no state dict, from a kernel bank that fails the constructor's own
// check, or on a machine without a device from the first upload) and must throw maa::Error.  Built alone with the host
// AddressSanitizer and linked against libaudiogpt_mi355x.so, the run ends with LeakSanitizer's report: no leak may name a
// maa:: frame.  Needs no device: the throw comes before (or from) the first device allocation.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer -g \
//       tests/native/unwind_main.cpp -o unwind_main -fsanitize=address -Laudiogpt_amd -laudiogpt_mi355x -Wl,-rpath,$PWD/audiogpt_amd
#include "../../audiogpt_amd/csrc/models.h"

#include <cstdio>
#include <vector>

namespace {

int failures = 0;

template <class F>
void expect_error(const char* what, F&& make) {
    try {
        make();
        std::printf("FAIL %s: constructed\n", what);
        ++failures;
    } catch (const maa::Error& e) {
        std::printf("ok   %s: %s\n", what, e.what());
    }
}

}  // namespace

int main() {
    const maa::StateDict empty;
    for (int precision = 0; precision <= 1; ++precision) {
        maa_unet_config u{};
        u.in_channels = u.out_channels = 4, u.model_channels = 32, u.num_res_blocks = 1, u.n_channel_mult = 1, u.channel_mult[0] = 1;
        u.num_heads = 1, u.num_head_channels = 32, u.transformer_depth = 1;
        expect_error("UNet", [&] { maa::UNet m(u, empty, precision); });
        maa_vae_config v{};
        v.ch = 32, v.out_ch = 1, v.in_channels = 1, v.z_channels = 4, v.embed_dim = 4, v.resolution = 16, v.num_res_blocks = 1;
        v.double_z = 1, v.n_ch_mult = 1, v.ch_mult[0] = 1;
        expect_error("VAE", [&] { maa::VAE m(v, empty, precision); });
        maa_vocoder_config g{};
        g.num_mels = 80, g.upsample_initial_channel = 32, g.n_upsamples = 1, g.upsample_rates[0] = 2, g.upsample_kernel_sizes[0] = 4;
        g.n_kernels = 1, g.resblock_kernel_sizes[0] = 3, g.n_dilations = 1, g.resblock_dilation_sizes[0][0] = 1, g.resblock = 1;
        expect_error("Vocoder", [&] { maa::Vocoder m(g, empty, precision); });
        maa_diffnet_config d{};
        d.in_dims = 80, d.hidden_size = 256, d.residual_layers = 2, d.residual_channels = 64, d.dilation_cycle_length = 1;
        expect_error("DiffNet", [&] { maa::DiffNet m(d, empty, precision); });
        maa_pitch_extractor_config p{};
        p.n_mel_bins = 80, p.hidden_size = 64, p.predictor_hidden = -1, p.predictor_kernel = 5, p.conv_layers = 2, p.ffn_padding_same = 1;
        p.use_uv = 1, p.f0_std = 1.f;
        expect_error("PitchExtractor", [&] { maa::PitchExtractor m(p, empty, precision); });
        maa_fs2_config f{};
        f.vocab_size = 16, f.hidden_size = 128, f.enc_layers = 1, f.dec_layers = 1, f.num_heads = 1, f.enc_ffn_kernel_size = 9;
        f.dec_ffn_kernel_size = 9, f.dur_predictor_layers = 1, f.dur_predictor_kernel = 3, f.predictor_hidden = -1, f.audio_num_mel_bins = 80;
        f.ffn_padding_same = f.ffn_act_gelu = f.dur_loss_mse = f.rel_pos = f.use_pos_embed = f.encoder_fft = f.decoder_fft = 1;
        expect_error("FastSpeech2MIDI", [&] { maa::FastSpeech2MIDI m(f, empty, precision); });
        maa_fs2_pitch_config fp{};
        fp.hidden_size = 128, fp.predictor_hidden = -1, fp.predictor_layers = 1, fp.predictor_kernel = 5, fp.ffn_padding_same = 1;
        fp.pitch_type_frame = 1, fp.use_uv = 1, fp.f0_std = 1.f;
        expect_error("FS2Pitch", [&] { maa::FS2Pitch m(fp, empty, precision); });
        for (int kind = 0; kind <= 2; ++kind) {
            maa_encoder_config e{};
            e.kind = kind, e.layers = 1, e.width = 64, e.heads = 1, e.mlp_dim = 128, e.d_proj = 64, e.vocab = 16, e.max_positions = 8;
            e.patch = 4, e.image = 8, e.ln_eps = 1e-5f;
            expect_error("Encoder", [&] { maa::Encoder m(e, empty, precision); });
        }
        maa_clap_audio_config c{};
        c.mel_bins = 64, c.n_blocks = 1, c.channels[0] = 32, c.out_emb = 64, c.d_proj = 64, c.bn_eps = 1e-5f;
        expect_error("ClapAudio", [&] { maa::ClapAudio m(c, empty, precision); });
    }
    // no state dict: the resampler's own check on the bank's length throws after Impl exists; the front end's first upload
    // throws where there is no device (with one it constructs, which is no failure of the unwinding)
    std::vector<float> bank(64, 0.f);
    expect_error("Resampler", [&] { maa::Resampler m(2, 1, 3, 7, bank.data()); });
    maa_spectral_config s{};
    s.n_fft = 8, s.hop = 4, s.n_freq = 5, s.n_mels = 2, s.power = 1, s.amin = 1e-5f, s.ref = 1.f;
    std::vector<float> basis(2 * 5 * 8, 0.f), melw(2 * 5, 0.f);
    try {
        maa::Spectral m(s, basis.data(), melw.data());
        std::printf("ok   Spectral: constructed (a device is present)\n");
    } catch (const maa::Error& e) {
        std::printf("ok   Spectral: %s\n", e.what());
    }
    std::printf("%s\n", failures ? "UNWIND_FAILED" : "UNWIND_OK");
    return failures ? 1 : 0;
}
