// Row kernels of DiffSinger's FastSpeech2MIDI front end (score -> decoder_inp, mel2ph, coarse mel), channels-last [B*T, C],
// wave64: one wave per row, four channels per lane per step; reductions are wave shuffles.  The contractions between them are
// fs2.cpp's; the masked attention is flash_attn.hip (bf16 modes) or blocks.cpp's three launches (exact fp32).
//
// Replaces (NeuralSeq/): modules/diffsinger_midi/fs2.py:12-23,60-65 the four embeddings with
// modules/commons/espnet_positional_embedding.py:102-113 RelPositionalEncoding and tts_modules.py:314,320 the first mask;
// tts_modules.py:98-118 the duration predictor's last LayerNorm, Linear(C, 1), mask and out2dur; :204-214 LengthRegulator;
// modules/fastspeech/fs2.py:117-122,132 expand + mask of the encoder states; and, for the cascade configurations
// (use_pitch_embed), fs2.py:187-220 the pitch tail: the predictor's last LayerNorm + Linear(C, 2), denorm_f0,
// utils/pitch_utils.py:15-31 f0_to_coarse, the pitch_embed gather and the mask, one launch.
// and, for the plain FastSpeech2 (modules/fastspeech/fs2.py; tts_modules.py:365-375), the token-counted positions and the
// embedding with the scale applied once, the speaker gather and broadcast add (fs2.py:96-125), and the energy tail (fs2.py:132,
// 165-172): the predictor's last LayerNorm + Linear(C, 1), the bin, the energy_embed gather, the speaker add and the mask, one launch.
// All of them are memory-bound on a few hundred to a few thousand rows.
// The launch grid and the duration head's LayerNorm + Linear stage are row_device.h's, shared with norm.hip's LayerNorm and
// pitch.hip's head; the decoder's masks, masked products and positional add are pitch.hip's launches (models.h).
#include "maa_internal.h"
#include "row_device.h"

#include <cmath>

namespace maa {
namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// x = ((scale * E[tok] + M[midi] + (dur * w + b) + S[slur]) * scale + pe[t]) * live,  live = tok != 0: the embedding scale is
// applied twice, as the reference does (forward_embedding's embed_scale, then RelPositionalEncoding's xscale).
// nonpad[row] = live, hidden[row] = 1 - live (the key mask of the attention).  midi_dur / is_slur may be null: their term is 0.
__global__ __launch_bounds__(256) void fs2_embed_kernel(const int* __restrict__ tok, const int* __restrict__ midi,
                                                        const float* __restrict__ midi_dur, const int* __restrict__ slur,
                                                        const float* __restrict__ E, int vocab, const float* __restrict__ Mi,
                                                        const float* __restrict__ dw, const float* __restrict__ db,
                                                        const float* __restrict__ S, const float* __restrict__ pe, float scale,
                                                        long long rows, int T, int H, float* __restrict__ x,
                                                        float* __restrict__ nonpad, float* __restrict__ hidden) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int t = (int)(row % T);
    const int tk = tok[row];
    const float live = tk != 0 ? 1.f : 0.f;
    const float* e = E + (long long)clampi(tk, 0, vocab - 1) * H;
    const float* m = Mi + (long long)clampi(midi[row], 0, 299) * H;
    const float* s = slur ? S + (long long)clampi(slur[row], 0, 1) * H : nullptr;
    const float d = midi_dur ? midi_dur[row] : 0.f;
    const float* p = pe + (long long)t * H;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 ev = *reinterpret_cast<const float4*>(e + c);
        const float4 mv = *reinterpret_cast<const float4*>(m + c);
        const float4 pv = *reinterpret_cast<const float4*>(p + c);
        float4 v = make_float4(scale * ev.x + mv.x, scale * ev.y + mv.y, scale * ev.z + mv.z, scale * ev.w + mv.w);
        if (midi_dur) {
            const float4 w = *reinterpret_cast<const float4*>(dw + c);
            const float4 b = *reinterpret_cast<const float4*>(db + c);
            v.x += d * w.x + b.x;
            v.y += d * w.y + b.y;
            v.z += d * w.z + b.z;
            v.w += d * w.w + b.w;
        }
        if (s) {
            const float4 sv = *reinterpret_cast<const float4*>(s + c);
            v.x += sv.x;
            v.y += sv.y;
            v.z += sv.z;
            v.w += sv.w;
        }
        v.x = (v.x * scale + pv.x) * live;
        v.y = (v.y * scale + pv.y) * live;
        v.z = (v.z * scale + pv.z) * live;
        v.w = (v.w * scale + pv.w) * live;
        *reinterpret_cast<float4*>(x + row * H + c) = v;
    }
    if (lane == 0) {
        nonpad[row] = live;
        hidden[row] = 1.f - live;
    }
}

// out2dur: max(rint(exp(xs) - 1), 0) (torch.round = half to even)
__device__ __forceinline__ int fs2_out2dur(float xs) { return (int)fmaxf(rintf(expf(xs) - 1.f), 0.f); }

// The duration predictor's last layer after its convolution (whose epilogue did the ReLU): LayerNorm over the row (kept in
// registers, C <= 256 * NR), mask, Linear(C, 1) (row_device.h), mask -> xs[row]; dur[row] = out2dur(xs).  A padding row is 0 in
// both.
template <int NR>
__global__ __launch_bounds__(256) void fs2_dur_head_kernel(const float* __restrict__ x, long long rows, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ nonpad, float* __restrict__ xs,
                                                           int* __restrict__ dur) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float d[1];
    ln_head_dots<NR, 1>(x + row * C, C, lane, gamma, beta, eps, w, bias, d);
    if (lane == 0) {
        const float o = nonpad[row] != 0.f ? d[0] : 0.f;
        xs[row] = o;
        dur[row] = fs2_out2dur(o);
    }
}

// LengthRegulator, one block per sample.  The inclusive running sum of dur[b, :] goes to cum[b, :] (256 tokens per step: a scan
// inside each wave, the waves' sums through LDS, the carry in a register); totals[b] = its last value, when asked for.
// mel2ph, when asked for: frame p belongs to the first token whose running sum exceeds p (1-based), 0 from the total on.
__global__ __launch_bounds__(256) void fs2_length_kernel(const int* __restrict__ dur, int T, int* cum,
                                                         int* __restrict__ totals, int T_mel, int* __restrict__ mel2ph) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int* src = dur + (long long)blockIdx.x * T;
    int* cs = cum + (long long)blockIdx.x * T;
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        int v = t < T ? src[t] : 0;
        v = v > 0 ? v : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        __syncthreads();
        if (lane == 63) wsum[w] = v;
        __syncthreads();
        int before = carry;
        for (int i = 0; i < w; ++i) before += wsum[i];
        if (t < T) cs[t] = before + v;
        carry += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
    if (totals && threadIdx.x == 0) totals[blockIdx.x] = carry;
    if (!mel2ph) return;
    __syncthreads();          // (block-wide: cum[b, :] written above is read below by other threads)
    int* dst = mel2ph + (long long)blockIdx.x * T_mel;
    for (int p = threadIdx.x; p < T_mel; p += 256) {
        int lo = 0, hi = T;      // first t in [0, T) with cs[t] > p; T: none
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cs[mid] > p) hi = mid;
            else lo = mid + 1;
        }
        dst[p] = lo < T ? lo + 1 : 0;
    }
}

// decoder_inp[b, p] = encoder_out[b, mel2ph[b, p] - 1] where mel2ph > 0, else 0; tgt[b, p] = (mel2ph > 0)
__global__ __launch_bounds__(256) void fs2_expand_kernel(const float* __restrict__ enc, const int* __restrict__ mel2ph, long long rows,
                                                         int T, int T_mel, int H, float* __restrict__ out, float* __restrict__ tgt) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long b = row / T_mel;
    const int ph = clampi(mel2ph[row], 0, T);
    const float* src = enc + (b * T + (ph > 0 ? ph - 1 : 0)) * H;
    for (int c = lane * 4; c < H; c += 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ph > 0) v = *reinterpret_cast<const float4*>(src + c);
        *reinterpret_cast<float4*>(out + row * H + c) = v;
    }
    if (lane == 0) tgt[row] = ph > 0 ? 1.f : 0.f;
}

// tgt[i] = (mel2ph[i] > 0): run_decoder's last mask, where no expand has made it
__global__ __launch_bounds__(256) void fs2_tgt_mask_kernel(const int* __restrict__ mel2ph, long long rows, float* __restrict__ tgt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < rows) tgt[i] = mel2ph[i] > 0 ? 1.f : 0.f;
}

// f0_to_coarse (utils/pitch_utils.py:15-31) in fp32, in the reference's operation order: mel_min = 1127 ln(1 + 50 / 700) and
// mel_span = 1127 ln(1 + 1100 / 700) - mel_min arrive rounded to fp32, as torch rounds the Python scalars.  Always in [1, 255]
// (a NaN lands in bin 1), so the table read below stays inside its 300 rows.
__device__ __forceinline__ int fs2_f0_to_coarse(float f0, float mel_min, float mel_span) {
    float m = 1127.f * logf(1.f + f0 / 700.f);
    if (m > 0.f) m = (m - mel_min) * 254.f / mel_span + 1.f;
    if (!(m > 1.f)) m = 1.f;
    if (m > 255.f) m = 255.f;
    return (int)(m + 0.5f);
}

// add_pitch after the predictor's last convolution (modules/fastspeech/fs2.py:187-220, pitch_type 'frame') and the mask of :132.
// Row r: LayerNorm (registers, C <= 256 * NR) and Linear(C, 2) -> {value, voicing logit}; f0 = f0_in[r] if given, else the value;
// with use_uv the frame is unvoiced where uv_in[r] > 0 if given, else where the logit is > 0 (the two inputs are independently
// nullable, :210-213); without use_uv no frame is, a caller's uv included (denorm_f0 reads it under hparams['use_uv'] only);
// denorm_f0 -> f0_denorm[r] (0 where unvoiced or mel2ph[r] == 0); f0_to_coarse -> coarse[r] (optional); then all lanes:
// decoder_inp[r, :] = (origin[r, :] + pitch_embed[coarse, :]) * (mel2ph[r] > 0).  Every lane holds the same dots, so nothing is
// broadcast and no [B, T] tensor goes through memory between the head and the gather.
// pitch_pred[r, 0] is 0 on a padding frame when f0 was predicted: the reference's `f0[pitch_padding] = 0` (:215-216) writes
// through the view f0 = pitch_pred[:, :, 0].  A caller's f0 is only read.
template <int NR>
__global__ __launch_bounds__(256) void fs2_pitch_tail_kernel(const float* __restrict__ x, long long rows, int C,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const int* __restrict__ mel2ph, const float* __restrict__ f0_in,
                                                             const float* __restrict__ uv_in, int norm, float f0_mean, float f0_std,
                                                             int use_uv, float mel_min, float mel_span,
                                                             const float* __restrict__ origin, const float* __restrict__ table, int H,
                                                             float* __restrict__ pitch_pred, float* __restrict__ f0_denorm,
                                                             int* __restrict__ coarse, float* __restrict__ decoder_inp) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float d[2];
    ln_head_dots<NR, 2>(x + row * C, C, lane, gamma, beta, eps, w, bias, d);
    const float live = mel2ph[row] > 0 ? 1.f : 0.f;
    const float f0 = f0_in ? f0_in[row] : d[0];
    const float uv = uv_in ? uv_in[row] : d[1];
    const float f = pe_denorm_f0(f0, uv, live, norm, f0_mean, f0_std, use_uv);
    const int bin = fs2_f0_to_coarse(f, mel_min, mel_span);
    if (lane == 0) {
        *reinterpret_cast<float2*>(pitch_pred + row * 2) = make_float2(f0_in || live != 0.f ? d[0] : 0.f, d[1]);
        f0_denorm[row] = f;
        if (coarse) coarse[row] = bin;
    }
    const float* e = table + (long long)bin * H;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 o = *reinterpret_cast<const float4*>(origin + row * H + c);
        const float4 p = *reinterpret_cast<const float4*>(e + c);
        *reinterpret_cast<float4*>(decoder_inp + row * H + c) =
            make_float4((o.x + p.x) * live, (o.y + p.y) * live, (o.z + p.z) * live, (o.w + p.w) * live);
    }
}

// ---- the plain FastSpeech2 (modules/fastspeech/fs2.py: the TTS configurations and both *_ds_beta6 chains)
// make_positions on the tokens (utils/__init__.py make_positions, padding_idx 0): pos[b, t] = #{t' <= t : tok[b, t'] != 0} where
// tok[b, t] != 0, else 0 -- a padding token inside a sample does not advance the count.  One block per sample, 256 tokens per
// step: a ballot per wave, the waves' counts through LDS, the running count carried in a register (as pitch.hip counts frames).
__global__ __launch_bounds__(256) void fs2_token_positions_kernel(const int* __restrict__ tok, int T, int* __restrict__ pos) {
    __shared__ int cnt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int* src = tok + (long long)blockIdx.x * T;
    int* dst = pos + (long long)blockIdx.x * T;
    int carry = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + (int)threadIdx.x;
        const bool nz = t < T && src[t] != 0;
        const unsigned long long bal = __ballot(nz);
        const int below = __popcll(bal & ((2ull << lane) - 1ull));          // lanes 0 .. lane, this one included
        __syncthreads();
        if (lane == 0) cnt[w] = __popcll(bal);
        __syncthreads();
        int before = carry;
        for (int i = 0; i < w; ++i) before += cnt[i];
        if (t < T) dst[t] = nz ? before + below : 0;
        carry += (cnt[0] + cnt[1]) + (cnt[2] + cnt[3]);
    }
}

// FastspeechEncoder.forward_embedding (tts_modules.py:365-375) and FFTBlocks' first mask.  rel == 0: x = (scale * E[tok] +
// table[pos[row]]) * live, the scale applied once, the sinusoid row chosen by the counted position (at most T: the caller grew the
// table to T + 1 rows).  rel != 0: x = ((scale * E[tok]) * scale + pe[t]) * live, RelPositionalEncoding on the scaled embedding
// -- the MIDI form without its three note terms; pos is not read.  nonpad / hidden as fs2_embed_kernel.
__global__ __launch_bounds__(256) void fs2_embed_plain_kernel(const int* __restrict__ tok, const int* __restrict__ pos,
                                                              const float* __restrict__ E, int vocab, const float* __restrict__ pe,
                                                              float scale, int rel, long long rows, int T, int H,
                                                              float* __restrict__ x, float* __restrict__ nonpad,
                                                              float* __restrict__ hidden) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int tk = tok[row];
    const float live = tk != 0 ? 1.f : 0.f;
    const float* e = E + (long long)clampi(tk, 0, vocab - 1) * H;
    const float* p = pe + (long long)(rel ? (int)(row % T) : clampi(pos[row], 0, T)) * H;
    const float outer = rel ? scale : 1.f;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 ev = *reinterpret_cast<const float4*>(e + c);
        const float4 pv = *reinterpret_cast<const float4*>(p + c);
        float4 v;
        v.x = ((scale * ev.x) * outer + pv.x) * live;
        v.y = ((scale * ev.y) * outer + pv.y) * live;
        v.z = ((scale * ev.z) * outer + pv.z) * live;
        v.w = ((scale * ev.w) * outer + pv.w) * live;
        *reinterpret_cast<float4*>(x + row * H + c) = v;
    }
    if (lane == 0) {
        nonpad[row] = live;
        hidden[row] = 1.f - live;
    }
}

// out[r, :] = (x[r, :] + spk[r / T, :]) * live, live = mask[r] != 0 (encode's src_nonpadding) or mel2ph[r] > 0: the inputs of the
// duration, pitch and energy predictors (fs2.py:114, 125)
__global__ __launch_bounds__(256) void fs2_add_speaker_kernel(const float* __restrict__ x, const float* __restrict__ spk,
                                                              const int* __restrict__ mel2ph, const float* __restrict__ mask,
                                                              long long rows, int T, int H, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float live = (mask ? mask[row] != 0.f : mel2ph[row] > 0) ? 1.f : 0.f;
    const float* s = spk + (row / T) * H;
    for (int c = lane * 4; c < H; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(x + row * H + c);
        const float4 sv = *reinterpret_cast<const float4*>(s + c);
        *reinterpret_cast<float4*>(out + row * H + c) =
            make_float4((v.x + sv.x) * live, (v.y + sv.y) * live, (v.z + sv.z) * live, (v.w + sv.w) * live);
    }
}

// out[k, b, :] = tab_k[id, :] for k = 0, 1, 2 (spk, spk_dur, spk_f0).  ids given: id = ids[k, b] with split, ids[0, b] without
// (fs2.py:104-110), clamped into the n_rows rows; ids null: id = b, the three copies of a [B, H] projection (fs2.py:97)
__global__ __launch_bounds__(256) void fs2_speaker_gather_kernel(const float* __restrict__ t0, const float* __restrict__ t1,
                                                                 const float* __restrict__ t2, const int* __restrict__ ids, int split,
                                                                 int n_rows, int B, int H, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= 3LL * B) return;
    const int k = (int)(row / B), b = (int)(row % B);
    const float* tab = k == 0 ? t0 : k == 1 ? t1 : t2;
    const int id = ids ? clampi(ids[(split ? k : 0) * B + b], 0, n_rows - 1) : b;
    for (int c = lane * 4; c < H; c += 256)
        *reinterpret_cast<float4*>(out + row * H + c) = *reinterpret_cast<const float4*>(tab + (long long)id * H + c);
}

// The end of FastSpeech2.forward's variance stage (fs2.py:165-172, 132), one wave per frame.  With an energy branch (x given):
// the predictor's last LayerNorm (registers, C <= 256 * NR) and Linear(C, 1) -> energy_pred[r], on every frame as the reference
// returns it; e = energy_in[r] if given, else the prediction; bin = clamp(e * 256 // 4, max = 255) = floor(64 e) exactly in fp32,
// clamped to [0, 255] (the reference raises IndexError below 0; a NaN lands in bin 0) -> energy_bin[r] (optional); then all lanes:
// decoder_inp[r, :] = (acc[r, :] + energy_embed[bin, :] + spk[b, :]) * (mel2ph[r] > 0), summed in that order.  Every lane holds the
// same dot, so no [B, T] tensor goes through memory between the head and the gather.  Without an energy branch (x null) the same
// launch is (acc + spk[b]) * tgt; spk may be null too.
template <int NR>
__global__ __launch_bounds__(256) void fs2_energy_tail_kernel(const float* __restrict__ x, long long rows, int C,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const int* __restrict__ mel2ph, const float* __restrict__ energy_in,
                                                              const float* __restrict__ acc, const float* __restrict__ table,
                                                              const float* __restrict__ spk, int T_mel, int H,
                                                              float* __restrict__ energy_pred, int* __restrict__ energy_bin,
                                                              float* __restrict__ decoder_inp) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float live = mel2ph[row] > 0 ? 1.f : 0.f;
    const float* e = nullptr;
    if (x) {
        float d[1];
        ln_head_dots<NR, 1>(x + row * C, C, lane, gamma, beta, eps, w, bias, d);
        const float q = floorf((energy_in ? energy_in[row] : d[0]) * 64.f);
        const int bin = q >= 255.f ? 255 : q > 0.f ? (int)q : 0;
        if (lane == 0) {
            if (energy_pred) energy_pred[row] = d[0];
            if (energy_bin) energy_bin[row] = bin;
        }
        e = table + (long long)bin * H;
    }
    const float* s = spk ? spk + (row / T_mel) * H : nullptr;
    for (int c = lane * 4; c < H; c += 256) {
        float4 v = *reinterpret_cast<const float4*>(acc + row * H + c);
        if (e) {
            const float4 p = *reinterpret_cast<const float4*>(e + c);
            v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
        }
        if (s) {
            const float4 p = *reinterpret_cast<const float4*>(s + c);
            v.x += p.x, v.y += p.y, v.z += p.z, v.w += p.w;
        }
        *reinterpret_cast<float4*>(decoder_inp + row * H + c) = make_float4(v.x * live, v.y * live, v.z * live, v.w * live);
    }
}

}  // namespace

void launch_fs2_embed(const Ctx& ctx, const int* tok, const int* midi, const float* midi_dur, const int* slur, const float* E, int vocab,
                      const float* Mi, const float* dw, const float* db, const float* S, const float* pe, float scale, int B, int T, int H,
                      float* x, float* nonpad, float* hidden) {
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "FastSpeech2MIDI: hidden_size must be a multiple of 4");
    const long long rows = (long long)B * T;
    ProfScope prof(ctx, "fs2_rows", 0.0, 20.0 * rows * (double)H);
    hipLaunchKernelGGL(fs2_embed_kernel, row_grid(rows), dim3(256), 0, ctx.stream, tok, midi, midi_dur, slur, E, vocab, Mi, dw, db, S, pe,
                       scale, rows, T, H, x, nonpad, hidden);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_dur_head(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                         const float* w, const float* bias, const float* nonpad, float* xs, int* dur) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0 && C <= 1024, "FastSpeech2MIDI: predictor width must be a multiple of 4, at most 1024");
    ProfScope prof(ctx, "fs2_rows", 0.0, 4.0 * rows * (double)C);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, row_grid(rows), dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, w, bias, nonpad, xs, dur);
    };
    if (C <= 256)
        go(fs2_dur_head_kernel<1>);
    else if (C <= 512)
        go(fs2_dur_head_kernel<2>);
    else
        go(fs2_dur_head_kernel<4>);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_length(Ctx& ctx, const int* dur, int B, int T, int* totals, int T_mel, int* mel2ph) {
    int* cum = reinterpret_cast<int*>(ctx.ws.alloc_f((size_t)B * T));
    if (ctx.ws.dry) return;
    ProfScope prof(ctx, "fs2_rows", 0.0, 8.0 * B * ((double)T + T_mel));
    hipLaunchKernelGGL(fs2_length_kernel, dim3((unsigned)B), dim3(256), 0, ctx.stream, dur, T, cum, totals, T_mel, mel2ph);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_expand(const Ctx& ctx, const float* enc, const int* mel2ph, int B, int T, int T_mel, int H, float* out, float* tgt) {
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "FastSpeech2MIDI: hidden_size must be a multiple of 4");
    const long long rows = (long long)B * T_mel;
    ProfScope prof(ctx, "fs2_rows", 0.0, 8.0 * rows * (double)H);
    hipLaunchKernelGGL(fs2_expand_kernel, row_grid(rows), dim3(256), 0, ctx.stream, enc, mel2ph, rows, T, T_mel, H, out, tgt);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_tgt_mask(const Ctx& ctx, const int* mel2ph, long long rows, float* tgt) {
    if (ctx.ws.dry) return;
    ProfScope prof(ctx, "fs2_rows", 0.0, 8.0 * rows);
    hipLaunchKernelGGL(fs2_tgt_mask_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx.stream, mel2ph, rows, tgt);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_pitch_tail(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                           const float* w, const float* bias, const int* mel2ph, const float* f0_in, const float* uv_in, int norm,
                           float f0_mean, float f0_std, int use_uv, const float* origin, const float* table, int H, float* pitch_pred,
                           float* f0_denorm, int* coarse, float* decoder_inp) {
    if (ctx.ws.dry) return;
    MAA_CHECK(C % 4 == 0 && C <= 1024, "FastSpeech2MIDI pitch: predictor width must be a multiple of 4, at most 1024");
    MAA_CHECK(H % 4 == 0, "FastSpeech2MIDI pitch: hidden_size must be a multiple of 4");
    // f0_mel_min and f0_mel_max - f0_mel_min of pitch_utils.py:15-19 (f0_min 50, f0_max 1100), double there, fp32 in the tensor op
    const double mel_lo = 1127.0 * std::log(1.0 + 50.0 / 700.0), mel_hi = 1127.0 * std::log(1.0 + 1100.0 / 700.0);
    const float mel_min = (float)mel_lo, mel_span = (float)(mel_hi - mel_lo);
    ProfScope prof(ctx, "fs2_rows", 0.0, 4.0 * rows * ((double)C + 3.0 * H));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, row_grid(rows), dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, w, bias, mel2ph, f0_in, uv_in, norm,
                           f0_mean, f0_std, use_uv, mel_min, mel_span, origin, table, H, pitch_pred, f0_denorm, coarse, decoder_inp);
    };
    if (C <= 256)
        go(fs2_pitch_tail_kernel<1>);
    else if (C <= 512)
        go(fs2_pitch_tail_kernel<2>);
    else
        go(fs2_pitch_tail_kernel<4>);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_embed_plain(Ctx& ctx, const int* tok, const float* E, int vocab, const float* pe, float scale, int rel, int B, int T,
                            int H, float* x, float* nonpad, float* hidden) {
    const long long rows = (long long)B * T;
    int* pos = rel ? nullptr : reinterpret_cast<int*>(ctx.ws.alloc_f((size_t)rows));
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "FastSpeech2: hidden_size must be a multiple of 4");
    ProfScope prof(ctx, "fs2_rows", 0.0, 12.0 * rows * (double)H);
    if (!rel) hipLaunchKernelGGL(fs2_token_positions_kernel, dim3((unsigned)B), dim3(256), 0, ctx.stream, tok, T, pos);
    hipLaunchKernelGGL(fs2_embed_plain_kernel, row_grid(rows), dim3(256), 0, ctx.stream, tok, pos, E, vocab, pe, scale, rel, rows, T, H, x,
                       nonpad, hidden);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_add_speaker(const Ctx& ctx, const float* x, const float* spk, const int* mel2ph, const float* mask, int B, int T, int H,
                            float* out) {
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "FastSpeech2: hidden_size must be a multiple of 4");
    const long long rows = (long long)B * T;
    ProfScope prof(ctx, "fs2_rows", 0.0, 8.0 * rows * (double)H);
    hipLaunchKernelGGL(fs2_add_speaker_kernel, row_grid(rows), dim3(256), 0, ctx.stream, x, spk, mel2ph, mask, rows, T, H, out);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_speaker_gather(const Ctx& ctx, const float* t0, const float* t1, const float* t2, const int* ids, int split, int n_rows,
                               int B, int H, float* out) {
    if (ctx.ws.dry) return;
    MAA_CHECK(H % 4 == 0, "FastSpeech2: hidden_size must be a multiple of 4");
    ProfScope prof(ctx, "fs2_rows", 0.0, 24.0 * B * (double)H);
    hipLaunchKernelGGL(fs2_speaker_gather_kernel, row_grid(3LL * B), dim3(256), 0, ctx.stream, t0, t1, t2, ids, split, n_rows, B, H, out);
    MAA_HIP(hipGetLastError());
}

void launch_fs2_energy_tail(const Ctx& ctx, const float* x, long long rows, int C, const float* gamma, const float* beta, float eps,
                            const float* w, const float* bias, const int* mel2ph, const float* energy_in, const float* acc,
                            const float* table, const float* spk, int T_mel, int H, float* energy_pred, int* energy_bin,
                            float* decoder_inp) {
    if (ctx.ws.dry) return;
    MAA_CHECK(!x || (C % 4 == 0 && C <= 1024), "FastSpeech2 energy: predictor width must be a multiple of 4, at most 1024");
    MAA_CHECK(H % 4 == 0, "FastSpeech2: hidden_size must be a multiple of 4");
    ProfScope prof(ctx, "fs2_rows", 0.0, 4.0 * rows * ((x ? (double)C : 0.0) + 3.0 * H));
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, row_grid(rows), dim3(256), 0, ctx.stream, x, rows, C, gamma, beta, eps, w, bias, mel2ph, energy_in, acc,
                           table, spk, T_mel, H, energy_pred, energy_bin, decoder_inp);
    };
    if (!x || C <= 256)
        go(fs2_energy_tail_kernel<1>);
    else if (C <= 512)
        go(fs2_energy_tail_kernel<2>);
    else
        go(fs2_energy_tail_kernel<4>);
    MAA_HIP(hipGetLastError());
}

}  // namespace maa
