"""Geometry and weighting of `split_input_params`, the reference's crop-and-stitch evaluation of a latent wider than the model
was trained on (`LatentDiffusion_audio.apply_model`, text_to_audio/Make_An_Audio/ldm/models/diffusion/ddpm_audio.py:561-662):

    the noisy latent is cut into overlapping crops of `ks` every `stride` positions (torch.nn.Unfold, :582-585), the UNet runs
    on every crop (:645), the outputs are multiplied by a border-distance weighting (:650), stitched with torch.nn.Fold and
    divided by the folded weighting (:654, get_fold_unfold :242-293).

This module is the host side: the crop counts (:250-251), the fp32 weighting table [kh * kw, L] formed with the same torch-CPU
arithmetic as `delta_border` (:212-224) / `get_weighting` (:226-240) -- so that it equals the reference's bit for bit -- and the
checks of everything the reference gets wrong silently or fails on late.  The device side is `maa_unet_forward_split` and the
split fields of `maa_ddim_args` (include/maa.h).

The dictionary is the reference's:
    ks, stride                                           (kh, kw), (sh, sw)
    clip_min_weight, clip_max_weight                     clip of the border distance inside a crop
    tie_braker, clip_min_tie_weight, clip_max_tie_weight the same distance over the grid of crops, multiplied in
    patch_distributed_vq, vqf                            decode_first_stage's own split (not supported: see plan())
"""
import torch

from .._lib import MaaError

KEYS = ("ks", "stride", "clip_min_weight", "clip_max_weight", "tie_braker", "clip_min_tie_weight", "clip_max_tie_weight",
        "patch_distributed_vq", "vqf")


def crop_counts(H, W, ks, stride):
    """ddpm_audio.py:250-251."""
    return (H - ks[0]) // stride[0] + 1, (W - ks[1]) // stride[1] + 1


def border_distance(h, w):
    """delta_border (ddpm_audio.py:212-224) over meshgrid (:205-210): each position's (y, x) as integers divided by the integer
    corner (h - 1, w - 1) -- torch's true division of two int64 tensors, an fp32 result -- then the smaller of the distances to
    the four borders: 0 at the border, up to 0.5 at the centre.  [h, w] fp32.  h == 1 or w == 1 divides 0 by 0: NaN throughout."""
    y = torch.arange(0, h).view(h, 1, 1).expand(h, w, 1)
    x = torch.arange(0, w).view(1, w, 1).expand(h, w, 1)
    pos = torch.cat([y, x], dim=-1) / torch.tensor([h - 1, w - 1]).view(1, 1, 2)
    near = torch.min(pos, dim=-1, keepdim=True)[0]
    far = torch.min(1 - pos, dim=-1, keepdim=True)[0]
    return torch.min(torch.cat([near, far], dim=-1), dim=-1)[0]


def weighting(params, kh, kw, Ly, Lx):
    """get_weighting (ddpm_audio.py:226-240) as a [kh * kw, Ly * Lx] fp32 table: row p = y * kw + x of the crop, column l = ly *
    Lx + lx (the reference's [1, kh * kw, L] without its leading axis)."""
    w = torch.clip(border_distance(kh, kw), params["clip_min_weight"], params["clip_max_weight"])
    w = w.reshape(kh * kw, 1).repeat(1, Ly * Lx)
    if params["tie_braker"]:
        tie = torch.clip(border_distance(Ly, Lx), params["clip_min_tie_weight"], params["clip_max_tie_weight"])
        w = w * tie.reshape(1, Ly * Lx)
    return w.to(torch.float32).contiguous()


class SplitPlan(object):
    """What one (dictionary, latent size) pair comes to: kh, kw, sh, sw, Ly, Lx, L and `weight` [kh * kw, L] fp32 on the CPU."""

    def __init__(self, kh, kw, sh, sw, Ly, Lx, weight):
        self.kh, self.kw, self.sh, self.sw, self.Ly, self.Lx, self.L, self.weight = kh, kw, sh, sw, Ly, Lx, Ly * Lx, weight


def unet_down_factor(unet_cfg):
    """Total downsampling of a UNetModel: one stride-2 step between consecutive entries of channel_mult (openaimodel.py:575-600)."""
    return 2 ** (len(unet_cfg["channel_mult"]) - 1)


def plan(params, H, W, down=1, conditioning_key="crossattn"):
    """Check the reference's dictionary against an [*, *, H, W] latent and return its SplitPlan.  `down`: the UNet's total
    downsampling factor; `conditioning_key`: the model's.  Raises MaaError (NotImplementedError for patch_distributed_vq) with
    the reason; each case is one the reference computes nonsense for or fails on inside torch:

      * conditioning_key "concat": apply_model hands every crop the full-size concat tensor (:641-645) and DiffusionWrapper's
        torch.cat([x] + c_concat, dim=1) fails on the widths -- only the cross-attention models (T2A, I2A) can be split;
      * ks larger than the latent: the crop counts (:250-251) come to <= 0;
      * (H - kh) % sh or (W - kw) % sw != 0: Fold leaves the positions no crop covers at 0 in both the stitched output and the
        normalisation, and :654 divides 0 by 0 there;
      * kh < 2 or kw < 2: delta_border divides by kh - 1 / kw - 1;
      * a weighting that is not finite: with tie_braker and one row or one column of crops delta_border(Ly, Lx) is 0 / 0, the
        whole table NaN and so is every output of the reference;
      * kh or kw not divisible by the UNet's downsampling factor: the skip connections' sizes disagree inside the UNet;
      * patch_distributed_vq: decode_first_stage's branch builds its Fold from kernel_size[0] twice (:267) and cannot stitch a
        crop that is not square; the wide latent is decoded whole, as the reference does without the flag.
    """
    if not isinstance(params, dict):
        raise MaaError("split_input_params must be the reference's dictionary (keys %s), got %r" % (", ".join(KEYS), type(params)))
    missing = [k for k in ("ks", "stride", "clip_min_weight", "clip_max_weight", "tie_braker") if k not in params]
    if params.get("tie_braker"):
        missing += [k for k in ("clip_min_tie_weight", "clip_max_tie_weight") if k not in params]
    if missing:
        raise MaaError("split_input_params lacks %s (get_weighting reads them, ddpm_audio.py:226-240)" % ", ".join(missing))
    if params.get("patch_distributed_vq"):
        raise NotImplementedError(
            "split_input_params: patch_distributed_vq is not supported -- the reference's decode_first_stage branch builds its Fold "
            "from kernel_size[0] twice (ddpm_audio.py:267) and cannot stitch a mel crop that is not square; leave the flag false and "
            "the wide latent is decoded whole")
    if conditioning_key == "concat":
        raise MaaError("split_input_params: a concat-conditioned model cannot be split -- the reference hands every crop the "
                       "full-size concat tensor and fails in torch.cat (ddpm_audio.py:641-645); only the cross-attention models "
                       "(T2A, I2A) support it")
    try:
        (kh, kw), (sh, sw) = (int(v) for v in params["ks"]), (int(v) for v in params["stride"])
    except (TypeError, ValueError):
        raise MaaError("split_input_params: ks and stride must be pairs of integers, got %r / %r" % (params["ks"], params["stride"]))
    H, W = int(H), int(W)
    if kh < 2 or kw < 2:
        raise MaaError("split_input_params: ks %s must be at least 2 x 2 -- delta_border divides by ks - 1 (ddpm_audio.py:219-220)"
                       % ((kh, kw),))
    if sh < 1 or sw < 1:
        raise MaaError("split_input_params: stride %s must be positive" % ((sh, sw),))
    if kh > H or kw > W:
        raise MaaError("split_input_params: ks %s is larger than the latent %s -- the reference's crop count (ddpm_audio.py:250-251) "
                       "is not positive" % ((kh, kw), (H, W)))
    if (sh > kh and H > kh) or (sw > kw and W > kw):
        raise MaaError("split_input_params: stride %s larger than ks %s leaves gaps between the crops -- Fold leaves those "
                       "positions at 0 and the reference divides 0 by 0 there (ddpm_audio.py:654)" % ((sh, sw), (kh, kw)))
    if (H - kh) % sh or (W - kw) % sw:
        raise MaaError("split_input_params: ks %s with stride %s leaves part of the latent %s uncovered ((H - kh) %% sh = %d, "
                       "(W - kw) %% sw = %d) -- Fold leaves those positions at 0 and the reference divides 0 by 0 there "
                       "(ddpm_audio.py:654)" % ((kh, kw), (sh, sw), (H, W), (H - kh) % sh, (W - kw) % sw))
    if kh % down or kw % down:
        raise MaaError("split_input_params: ks %s must be divisible by the UNet's downsampling factor %d" % ((kh, kw), down))
    Ly, Lx = crop_counts(H, W, (kh, kw), (sh, sw))
    wt = weighting(params, kh, kw, Ly, Lx)
    if not bool(torch.isfinite(wt).all()):
        why = ""
        if params["tie_braker"] and (Ly == 1 or Lx == 1):
            why = (": tie_braker with Ly = %d, Lx = %d -- delta_border(Ly, Lx) divides 0 by 0 for a single row or column of crops "
                   "(the audio case, Ly == 1) and the reference's result is NaN throughout; set tie_braker to False" % (Ly, Lx))
        raise MaaError("split_input_params: the weighting is not finite" + why)
    return SplitPlan(kh, kw, sh, sw, Ly, Lx, wt)
