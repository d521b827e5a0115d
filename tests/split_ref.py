"""Test-side restatement of the `split_input_params` evaluation (LatentDiffusion_audio.apply_model,
ldm/models/diffusion/ddpm_audio.py:572-654) that the GPU tests compare against: torch's unfold, any per-crop model, and the
stitch  out = (sum_l w[p, l] * eps_l) / (sum_l w[p, l])  over the crops that cover a position in ascending l, in fp64.
tests/test_split_host.py pins it (over the CPU oracle's UNet) against the reference's own apply_model outputs."""
import numpy as np
import torch

# the golden script's cases and clip values (tests/golden/make_golden_split.py)
PARAMS = dict(clip_min_weight=0.01, clip_max_weight=0.5, tie_braker=False, clip_min_tie_weight=0.01, clip_max_tie_weight=0.5,
              patch_distributed_vq=False, vqf=8)
CASES = {
    "A": ((2, 4, 8, 40), (8, 16), (8, 8)),
    "B": ((1, 4, 12, 24), (8, 16), (4, 8)),
    "C": ((1, 4, 8, 32), (8, 16), (8, 16)),
    "D": ((1, 4, 8, 16), (8, 16), (8, 8)),
}


def params(case, tie=False):
    _, ks, stride = CASES[case]
    return dict(PARAMS, ks=ks, stride=stride, tie_braker=tie)


def unfold(x, ks, stride):
    """x [B, C, H, W] -> crops [B * L, C, kh, kw], row b * L + l (torch.nn.functional.unfold's columns as images)."""
    B, C = x.shape[:2]
    cols = torch.nn.functional.unfold(x, kernel_size=ks, stride=stride)          # [B, C * kh * kw, L]
    L = cols.shape[-1]
    return cols.reshape(B, C, ks[0], ks[1], L).permute(0, 4, 1, 2, 3).reshape(B * L, C, ks[0], ks[1]).contiguous()


def fold64(crops, weight, size, ks, stride):
    """crops [B * L, C, kh, kw], weight [kh * kw, L] (fp32 values) -> (out, bound) in fp64, each [B, C, H, W]:
    out = (sum_l w e) / norm, and bound = (n + 2) * 2^-24 * (sum_l |w e|) / norm with n the number of covering crops -- one
    rounding for the products (each on its own term), n - 1 for the sum, one for the fp32 value of norm, one for the division."""
    (H, W), (kh, kw), (sh, sw) = size, ks, stride
    Ly, Lx = (H - kh) // sh + 1, (W - kw) // sw + 1
    L = Ly * Lx
    e = torch.as_tensor(np.asarray(crops.detach().cpu() if torch.is_tensor(crops) else crops), dtype=torch.float64)
    w = torch.as_tensor(np.asarray(weight), dtype=torch.float64).reshape(kh, kw, L)
    B, C = e.shape[0] // L, e.shape[1]
    e = e.reshape(B, L, C, kh, kw)
    num, mag = torch.zeros(B, C, H, W, dtype=torch.float64), torch.zeros(B, C, H, W, dtype=torch.float64)
    norm, cnt = torch.zeros(H, W, dtype=torch.float64), torch.zeros(H, W, dtype=torch.float64)
    for l in range(L):
        y0, x0 = (l // Lx) * sh, (l % Lx) * sw
        term = e[:, l] * w[:, :, l]
        num[:, :, y0:y0 + kh, x0:x0 + kw] += term
        mag[:, :, y0:y0 + kh, x0:x0 + kw] += term.abs()
        norm[y0:y0 + kh, x0:x0 + kw] += w[:, :, l]
        cnt[y0:y0 + kh, x0:x0 + kw] += 1
    return num / norm, (cnt + 2) * 2.0 ** -24 * mag / norm


def apply_model_split(model, x, t, weight, ks, stride):
    """The split evaluation with `model(crops [n, C, kh, kw], t [n]) -> eps` run once per crop index, as the reference loops
    (ddpm_audio.py:645); returns the fp64 stitch."""
    B, _, H, W = x.shape
    z = unfold(x, ks, stride)
    L = z.shape[0] // B
    z = z.reshape(B, L, *z.shape[1:])
    outs = torch.stack([model(z[:, l].contiguous(), t) for l in range(L)], dim=1)          # [B, L, C, kh, kw]
    return fold64(outs.reshape(B * L, *outs.shape[2:]), weight, (H, W), ks, stride)[0]
