// The Glow post-net of GenerSpeech and PortaSpeech run in reverse on the device: latent z [B, T, C] + conditioning g [B, T, gin]
// -> mel x [B, 2 (T / 2), C] (AudioGPT's TTS_OOD and TTS tools; NeuralSeq/modules/GenerSpeech/model/generspeech.py:233-260).
//
// Mirrors modules/GenerSpeech/model/glow_modules.py:496-580 (Glow.forward, reverse), :282-332 (CouplingBlock), :114-189
// (InvConvNear), :68-91 (ActNorm), :742-767 (squeeze / unsqueeze) and model/wavenet.py:14-78 (WN).
// Layout: channels-last rows.  With n_sqz = 2 the reference's squeeze is a view of that layout -- squeezed row t' of a sample is
// [z[2t'], z[2t' + 1]], channel s * C + c -- so only the mask and the dropped odd frame cost a pass, and unsqueeze costs none:
// the last block writes the caller's x.  A Conv1d(k = 1) is a GEMM over the B * T_s rows, a dilated in_layer an implicit GEMM.
// Differences from a literal translation (same maths):
//   * the cond_layer convs of all blocks (one per block, or the one shared at Glow level) run as ONE GEMM per call,
//     [B T_s, 2 gin] x [2 gin, n_blocks 2H n_layers], and each layer's slice enters its in_layer as the igemm's residual term
//   * weight-norm pairs are folded at load (w = g v / |v| per output channel); plain `weight` keys, as after store_inverse, are taken
//     as they are
//   * with share_wn_layers = n the blocks of a group carry the same in_layers / res_skip_layers under their own keys: packed once
//     per group
//   * InvConvNear's weight is formed in fp32 as the reference forms it and inverted once, on the host, in float64
//   * the coupling tail, the 4 x 4 mix and ActNorm of a block are one launch (glow.hip), which also writes each row's share of
//     the coupling's log-determinant; a last kernel sums them per sample in a fixed order and adds the constant terms
// reverse issues launches on the context's stream only: no device-to-host copy, no synchronisation.
#include "models.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace maa {

maa_glow_config glow_resolved(const maa_glow_config& in) {
    maa_glow_config c = in;
    if (c.in_channels == 0) c.in_channels = 80;
    if (c.hidden_channels == 0) c.hidden_channels = 128;
    if (c.kernel_size == 0) c.kernel_size = 3;
    if (c.dilation_rate == 0) c.dilation_rate = 1;
    if (c.n_blocks == 0) c.n_blocks = 8;
    if (c.n_layers == 0) c.n_layers = 3;
    if (c.n_split == 0) c.n_split = 4;
    if (c.n_sqz == 0) c.n_sqz = 2;
    return c;
}

void check_glow_config(const maa_glow_config& raw) {
    const maa_glow_config c = glow_resolved(raw);
    MAA_CHECK(c.n_sqz == 2, "Glow: n_sqz must be 2 -- the squeeze is built as the pairing of neighbouring frames only");
    MAA_CHECK(c.n_split == 4, "Glow: n_split must be 4 -- InvConvNear is built as the 4 x 4 mix over channel groups only "
                              "(inv_conv_type 'near'; 'invconv' is not built)");
    MAA_CHECK(c.kernel_size >= 1 && c.kernel_size % 2 == 1, "Glow: kernel_size must be odd (WN asserts it: 'same' padding keeps the length only then)");
    MAA_CHECK(c.hidden_channels >= 2 && c.hidden_channels % 2 == 0, "Glow: hidden_channels must be even (WN asserts it)");
    MAA_CHECK(c.hidden_channels % 4 == 0 && c.hidden_channels <= 4096, "Glow: hidden_channels must be a multiple of 4 (16-byte accesses), at most 4096");
    MAA_CHECK(c.in_channels >= 4 && c.in_channels % 4 == 0 && c.in_channels <= 4096,
              "Glow: in_channels % 4 != 0 -- in_channels must be a multiple of 4 (16-byte accesses; the 4 x 4 mix stays inside a lane), at most 4096");
    MAA_CHECK(c.dilation_rate >= 1 && c.n_blocks >= 1 && c.n_blocks <= 64 && c.n_layers >= 1 && c.n_layers <= 16,
              "bad Glow config: dilation_rate >= 1, 1 <= n_blocks <= 64, 1 <= n_layers <= 16");
    MAA_CHECK(std::pow((double)c.dilation_rate, c.n_layers - 1) * (c.kernel_size - 1) / 2 < 65536.0, "bad Glow config: the last layer's dilation is too wide");
    MAA_CHECK(c.gin_channels >= 0 && c.gin_channels % 4 == 0 && c.gin_channels <= 16384,
              "Glow: gin_channels must be 0 (no conditioning) or a multiple of 4 (16-byte accesses), at most 16384");
    MAA_CHECK(c.share_wn_layers >= 0, "bad Glow config: share_wn_layers < 0");
}

void check_glow_reverse_args(const void* glow, const float* d_z, int B, int T, const float* d_x) {
    MAA_CHECK(glow && d_z && d_x, "bad glow_reverse arguments: null pointer");
    MAA_CHECK(B >= 1 && T >= 1 && (long long)B * T < (1LL << 31) / 8192, "bad glow_reverse arguments: B, T");
}

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// A state dict of plain weights: `prefix`weight as it is, or folded from `prefix`weight_g / weight_v (torch weight_norm, dim 0:
// w[o] = g[o] * v[o] / |v[o]|, the norm over everything but the output channel).
struct Folded {
    StateDict sd;
    std::map<std::string, std::vector<float>> store;

    std::string weight(const StateDict& src, const std::string& prefix) {
        const std::string name = prefix + "weight";
        if (sd.count(name)) return name;
        if (has(src, name)) {
            sd[name] = get(src, name);
            return name;
        }
        const HostTensor &g = get(src, prefix + "weight_g"), &v = get(src, prefix + "weight_v");
        MAA_CHECK(!v.shape.empty() && v.shape[0] > 0 && g.numel() == v.shape[0], "Glow: weight_g / weight_v shapes of " + prefix);
        const long long O = v.shape[0], per = v.numel() / O;
        std::vector<float>& w = store[name];
        w.resize((size_t)v.numel());
        for (long long o = 0; o < O; ++o) {
            double q = 0.0;
            for (long long i = 0; i < per; ++i) q += (double)v.data[o * per + i] * v.data[o * per + i];
            const double s = (double)g.data[o] / std::sqrt(q);
            for (long long i = 0; i < per; ++i) w[(size_t)(o * per + i)] = (float)(v.data[o * per + i] * s);
        }
        HostTensor h;
        h.data = w.data();
        h.shape = v.shape;
        sd[name] = h;
        return name;
    }
    std::string bias(const StateDict& src, const std::string& prefix) {
        const std::string name = prefix + "bias";
        if (!sd.count(name)) sd[name] = get(src, name);
        return name;
    }
};

bool same_tensor(const StateDict& sd, const std::string& a, const std::string& b) {
    if (has(sd, a) != has(sd, b)) return false;
    if (!has(sd, a)) return true;
    const HostTensor &x = get(sd, a), &y = get(sd, b);
    return x.shape == y.shape && std::memcmp(x.data, y.data, (size_t)x.numel() * sizeof(float)) == 0;
}

// the inverse of a 4 x 4 matrix by Gauss-Jordan with partial pivoting, float64
void invert4(const double* a, double* inv) {
    double m[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            m[i][j] = a[i * 4 + j];
            m[i][4 + j] = i == j ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(m[r][c]) > std::fabs(m[p][c])) p = r;
        MAA_CHECK(std::fabs(m[p][c]) > 0.0, "Glow: an InvConvNear weight is singular");
        if (p != c)
            for (int j = 0; j < 8; ++j) std::swap(m[p][j], m[c][j]);
        const double d = m[c][c];
        for (int j = 0; j < 8; ++j) m[c][j] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = m[r][c];
            for (int j = 0; j < 8; ++j) m[r][j] -= f * m[c][j];
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) inv[i * 4 + j] = m[i][4 + j];
}

}  // namespace

struct Glow::Impl {
    maa_glow_config cfg;
    int precision = 0;
    WeightStore ws;
    explicit Impl(int prec) : precision(prec), ws(prec != 0) {}
    struct Block {
        PackedW start, end;
        int wn = 0;                 // index of the group's WN in `in_layers` / `res_skip`
        float *winv = nullptr, *an_bias = nullptr, *an_einv = nullptr;
    };
    std::vector<Block> blocks;
    std::vector<std::vector<PackedW>> in_layers, res_skip;      // [group][layer]
    PackedW cond_all;               // every block's cond_layer on the N axis (share_cond_layers: the one of the Glow)
    double per_len = 0.0;           // the log-determinant per live squeezed row that does not depend on the data

    void build(const StateDict& sd) {
        const int C = cfg.in_channels, H = cfg.hidden_channels, L = cfg.n_layers, NB = cfg.n_blocks, k = cfg.kernel_size;
        const int share = cfg.share_wn_layers;
        Folded f;
        std::vector<std::string> cw, cb;
        for (int b = 0; b < NB; ++b) {
            const std::string pa = "flows." + std::to_string(3 * b) + ".", pi = "flows." + std::to_string(3 * b + 1) + ".",
                              pc = "flows." + std::to_string(3 * b + 2) + ".";
            Block blk;
            // ---- ActNorm
            const HostTensor &al = get(sd, pa + "logs"), &ab = get(sd, pa + "bias");
            MAA_CHECK(al.numel() == 2 * C && ab.numel() == 2 * C, "Glow ActNorm shape " + pa);
            std::vector<float> einv(2 * C), bias(ab.data, ab.data + 2 * C);
            for (int c = 0; c < 2 * C; ++c) {
                einv[c] = std::exp(-al.data[c]);
                per_len -= (double)al.data[c];
            }
            blk.an_einv = ws.upload(einv);
            blk.an_bias = ws.upload(bias);
            // ---- InvConvNear: W = P ((L o l_mask + I) (U o l_mask^T + diag(sign_s exp(log_s)))) in fp32 (_get_weight), inverse in float64
            {
                const HostTensor &p = get(sd, pi + "p"), &l = get(sd, pi + "l"), &u = get(sd, pi + "u"), &ls = get(sd, pi + "log_s"),
                                 &sg = get(sd, pi + "sign_s");
                MAA_CHECK(p.numel() == 16 && l.numel() == 16 && u.numel() == 16 && ls.numel() == 4 && sg.numel() == 4,
                          "Glow InvConvNear shape (n_split 4) " + pi);
                // (l_mask and eye are constant buffers of the module: the strict lower triangle and the identity)
                float lm[16], um[16], lu[16], w[16];
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) {
                        lm[i * 4 + j] = l.data[i * 4 + j] * (i > j ? 1.f : 0.f) + (i == j ? 1.f : 0.f);
                        um[i * 4 + j] = u.data[i * 4 + j] * (j > i ? 1.f : 0.f) + (i == j ? sg.data[i] * std::exp(ls.data[i]) : 0.f);
                    }
                auto mm = [](const float* a, const float* b, float* o) {
                    for (int i = 0; i < 4; ++i)
                        for (int j = 0; j < 4; ++j) {
                            float s = 0.f;
                            for (int q = 0; q < 4; ++q) s += a[i * 4 + q] * b[q * 4 + j];
                            o[i * 4 + j] = s;
                        }
                };
                mm(lm, um, lu);
                mm(p.data, lu, w);
                double wd[16], inv[16];
                for (int i = 0; i < 16; ++i) wd[i] = w[i];
                invert4(wd, inv);
                std::vector<float> winv(16);
                for (int i = 0; i < 16; ++i) winv[i] = (float)inv[i];
                blk.winv = ws.upload(winv);
                double s = 0.0;
                for (int i = 0; i < 4; ++i) s += (double)ls.data[i];
                per_len -= s * (2 * C / 4);
            }
            // ---- CouplingBlock
            blk.start = ws.pack_conv(f.sd, f.weight(sd, pc + "start."), f.bias(sd, pc + "start."), 1, 1);
            blk.end = ws.pack_conv(f.sd, f.weight(sd, pc + "end."), f.bias(sd, pc + "end."), 1, 1);
            MAA_CHECK(blk.start.K == C && blk.start.N == H && blk.end.K == H && blk.end.N == 2 * C, "Glow coupling start / end shape " + pc);
            const int lead = share > 0 ? b - b % share : b;      // the block whose keys the group's WN is packed from
            if (lead == b) {
                std::vector<PackedW> il, rl;
                for (int i = 0; i < L; ++i) {
                    const std::string pin = pc + "wn.in_layers." + std::to_string(i) + ".", prs = pc + "wn.res_skip_layers." + std::to_string(i) + ".";
                    il.push_back(ws.pack_conv(f.sd, f.weight(sd, pin), f.bias(sd, pin), 1, k));
                    rl.push_back(ws.pack_conv(f.sd, f.weight(sd, prs), f.bias(sd, prs), 1, 1));
                    MAA_CHECK(il.back().K == k * H && il.back().N == 2 * H, "Glow WN in_layer shape " + pin);
                    MAA_CHECK(rl.back().K == H && rl.back().N == (i + 1 < L ? 2 * H : H), "Glow WN res_skip_layer shape " + prs);
                }
                in_layers.push_back(std::move(il));
                res_skip.push_back(std::move(rl));
            } else {
                const std::string pl = "flows." + std::to_string(3 * lead + 2) + ".";
                for (int i = 0; i < L; ++i)
                    for (const char* layer : {"wn.in_layers.", "wn.res_skip_layers."})
                        for (const char* leaf : {".weight", ".weight_g", ".weight_v", ".bias"}) {
                            const std::string tail = layer + std::to_string(i) + leaf;
                            MAA_CHECK(same_tensor(sd, pc + tail, pl + tail),
                                      "Glow: share_wn_layers groups blocks whose " + tail + " differ (" + pc + " against " + pl + ")");
                        }
            }
            blk.wn = (int)in_layers.size() - 1;
            if (cfg.gin_channels > 0 && !cfg.share_cond_layers) {
                cw.push_back(f.weight(sd, pc + "wn.cond_layer."));
                cb.push_back(f.bias(sd, pc + "wn.cond_layer."));
            }
            blocks.push_back(blk);
        }
        if (cfg.gin_channels > 0) {
            if (cfg.share_cond_layers) {
                cw.push_back(f.weight(sd, "cond_layer."));
                cb.push_back(f.bias(sd, "cond_layer."));
            }
            cond_all = ws.pack_concat(f.sd, cw, cb);
            MAA_CHECK(cond_all.K == 2 * cfg.gin_channels && cond_all.N == (cfg.share_cond_layers ? 1 : NB) * 2 * H * L, "Glow cond_layer shape");
        }
    }

    void reverse(Ctx& ctx, const float* z, const float* g, const float* mask, int B, int T, float* x_out, float* logdet, float* hiddens) {
        const int C = cfg.in_channels, H = cfg.hidden_channels, L = cfg.n_layers, NB = cfg.n_blocks, k = cfg.kernel_size, gin = cfg.gin_channels;
        const int Ts = T / 2;
        const long long rows = (long long)B * Ts;
        float* mask_s = ctx.ws.alloc_f((size_t)rows);
        float* x = ctx.ws.alloc_f((size_t)rows * 2 * C);
        launch_glow_squeeze(ctx, z, mask, B, T, C, x, mask_s);
        // ---- conditioning of every block and layer: one GEMM
        const float* cond = nullptr;
        if (gin > 0) {
            float* gs = ctx.ws.alloc_f((size_t)rows * 2 * gin);
            launch_glow_squeeze(ctx, g, mask, B, T, gin, gs, nullptr);
            float* cc = ctx.ws.alloc_f((size_t)rows * cond_all.Npad);
            linear_into(ctx, gs, 2 * gin, rows, 2 * gin, cond_all, nullptr, 0, cc, cond_all.Npad);
            cond = cc;
        }
        float* h = ctx.ws.alloc_f((size_t)rows * H);
        float* y = ctx.ws.alloc_f((size_t)rows * 2 * H);
        float* a = ctx.ws.alloc_f((size_t)rows * H);
        float* skip = ctx.ws.alloc_f((size_t)rows * H);
        float* eo = ctx.ws.alloc_f((size_t)rows * 2 * C);
        float* rowld = ctx.ws.alloc_f((size_t)rows);
        const size_t hstride = (size_t)rows * 2 * C;
        for (int n = 0; n < NB; ++n) {
            const int b = NB - 1 - n;
            const Block& blk = blocks[b];
            // h = start(x0) * mask            (glow_modules.py:314-316)
            linear_into(ctx, x, 2 * C, rows, C, blk.start, nullptr, 0, h, H);
            launch_pe_affine_mask(ctx, h, rows, H, nullptr, nullptr, mask_s, h);
            // ---- WN (wavenet.py:54-78)
            int dil = 1;
            for (int i = 0; i < L; ++i) {
                const PackedW& w = in_layers[blk.wn][i];
                IGemm p;
                p.a1 = h;
                p.lda1 = H;
                p.C1 = H;
                p.Hin = p.Hout = 1;
                p.Win = p.Wout = Ts;
                p.KH = 1;
                p.KW = k;
                p.dw = dil;
                p.pw = (k * dil - dil) / 2;
                p.b = w.w;
                p.ldb = w.ld;
                p.b_nk = w.nk;
                p.b_split = w.split;
                p.M = (int)rows;
                p.K = k * H;
                p.N = 2 * H;
                p.bias = w.bias;
                if (cond) {      // g_l: this block's, this layer's 2H columns of the hoisted GEMM
                    p.res = cond + (size_t)((cfg.share_cond_layers ? 0 : b) * L + i) * 2 * H;
                    p.ldr = cond_all.Npad;
                }
                p.c = y;
                p.ldc = 2 * H;
                launch_igemm(ctx, p);
                launch_glow_gate(ctx, y, rows, H, a);
                const bool last = i + 1 == L;
                linear_into(ctx, a, H, rows, H, res_skip[blk.wn][i], nullptr, 0, y, last ? H : 2 * H);
                launch_glow_wn_residual(ctx, y, rows, H, mask_s, i == 0, last, h, skip);
                dil *= cfg.dilation_rate;
            }
            // out = end(o); coupling inverse, 4 x 4 mix, ActNorm: one launch; the last block writes the caller's x
            linear_into(ctx, skip, H, rows, H, blk.end, nullptr, 0, eo, 2 * C);
            float* hc = hiddens ? hiddens + (size_t)(3 * n) * hstride : nullptr;
            launch_glow_block_tail(ctx, x, eo, mask_s, rows, C, cfg.sigmoid_scale, blk.winv, blk.an_bias, blk.an_einv, n == 0,
                                   n + 1 == NB ? x_out : x, rowld, hc, hc ? hc + hstride : nullptr, hc ? hc + 2 * hstride : nullptr);
        }
        if (logdet) launch_glow_logdet(ctx, rowld, mask_s, B, Ts, (float)per_len, logdet);
    }
};

Glow::Glow(const maa_glow_config& cfg, const StateDict& sd, int precision) : impl_(new Impl(precision)) {
    check_glow_config(cfg);
    impl_->cfg = glow_resolved(cfg);
    impl_->build(sd);
}
Glow::~Glow() = default;
const maa_glow_config& Glow::config() const { return impl_->cfg; }

void Glow::reverse(Ctx& ctx, const float* z, const float* g, const float* mask, int B, int T, float* x, float* logdet, float* hiddens) {
    Impl& m = *impl_;
    MAA_CHECK(T >= 2, "glow_reverse: T < 2 -- the squeeze pairs frames, a single frame leaves no row");
    MAA_CHECK((g != nullptr) == (m.cfg.gin_channels > 0),
              "glow_reverse: d_g must be given exactly when the model has gin_channels > 0");
    MAA_CHECK(aligned16(z) && aligned16(x) && aligned16(g) && aligned16(hiddens), "glow_reverse: d_z, d_g, d_x and d_hiddens must be 16-byte aligned");
    MAA_CHECK(x != z, "glow_reverse: d_x may not alias d_z");
    PrecisionGuard pg(ctx, m.precision);
    run_sized(ctx, [&] { m.reverse(ctx, z, g, mask, B, T, x, logdet, hiddens); });
}

}  // namespace maa
