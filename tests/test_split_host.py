"""Host side of `split_input_params` (no GPU): audiogpt_amd/ldm/split.py against the reference's own weighting
(tests/golden/make_golden_split.py), its rejections, the test-side restatement of the split evaluation (tests/split_ref.py over
the CPU oracle's UNet) against the reference's apply_model, and the three new C entry points' binding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT
from audiogpt_amd._lib import MaaError
from audiogpt_amd.ldm import split as SP
from tests import split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = [("A", False), ("B", False), ("B", True), ("C", False), ("D", False)]


@pytest.mark.parametrize("case,tie", TAGS)
def test_weighting_and_crop_counts_equal_the_reference_bit_for_bit(golden, case, tie):
    g = golden("split_weights")
    shape, ks, stride = R.CASES[case]
    tag = case + ("_tie" if tie else "")
    p = SP.plan(R.params(case, tie), shape[2], shape[3], down=SP.unet_down_factor(C.UNET_T2A))
    assert [p.Ly, p.Lx, p.L] == g["L_" + tag].tolist()
    assert (p.kh, p.kw, p.sh, p.sw) == ks + stride
    w = p.weight.numpy()
    assert w.dtype == np.float32 and w.shape == g["w_" + tag].shape == (ks[0] * ks[1], p.L)
    assert np.array_equal(w.view(np.uint32), g["w_" + tag].view(np.uint32))
    # the reference's normalisation is the fold of that table (its fp32 sum against the fp64 one)
    n64 = np.zeros(shape[2:])
    for l in range(p.L):
        y0, x0 = (l // p.Lx) * stride[0], (l % p.Lx) * stride[1]
        n64[y0:y0 + ks[0], x0:x0 + ks[1]] += w[:, l].reshape(ks).astype(np.float64)
    assert np.abs(n64 - g["norm_" + tag]).max() <= 4 * 2.0 ** -24 * n64.max()


def _p(**kw):
    return dict(R.params("A"), **kw)


@pytest.mark.parametrize("params,hw,kw,exc,match", [
    (_p(ks=(16, 16)), (8, 40), {}, MaaError, "larger than the latent"),
    (_p(ks=(8, 48)), (8, 40), {}, MaaError, "larger than the latent"),
    (_p(stride=(8, 16)), (8, 40), {}, MaaError, "uncovered"),
    (_p(ks=(8, 16), stride=(3, 8)), (12, 40), {}, MaaError, "uncovered"),
    (_p(ks=(1, 16), stride=(1, 8)), (8, 40), {}, MaaError, "at least 2 x 2"),
    (_p(ks=(8, 1), stride=(8, 1)), (8, 40), {}, MaaError, "at least 2 x 2"),
    (_p(tie_braker=True), (8, 40), {}, MaaError, "not finite.*Ly = 1"),
    (dict(R.params("B", True), stride=(4, 8)), (12, 16), {}, MaaError, "not finite.*Lx = 1"),
    (_p(), (8, 40), dict(down=16), MaaError, "downsampling factor 16"),
    (_p(ks=(8, 10), stride=(8, 10)), (8, 40), dict(down=4), MaaError, "downsampling factor 4"),
    (_p(), (8, 40), dict(conditioning_key="concat"), MaaError, "concat.*torch.cat"),
    (_p(patch_distributed_vq=True), (8, 40), {}, NotImplementedError, r"ddpm_audio\.py:267"),
    (_p(clip_max_weight=float("nan")), (8, 40), {}, MaaError, "not finite"),
    (_p(ks=(8, 8), stride=(8, 16)), (8, 40), {}, MaaError, "gaps"),
])
def test_what_the_reference_cannot_compute_is_rejected_with_the_reason(params, hw, kw, exc, match):
    with pytest.raises(exc, match=match):
        SP.plan(params, hw[0], hw[1], **kw)


def test_missing_keys_and_a_non_dictionary_are_rejected():
    p = R.params("A")
    del p["clip_min_weight"]
    with pytest.raises(MaaError, match="clip_min_weight"):
        SP.plan(p, 8, 40)
    with pytest.raises(MaaError, match="dictionary"):
        SP.plan([8, 16], 8, 40)


@pytest.mark.parametrize("case,tie", [("A", False), ("B", False), ("B", True)])
def test_restatement_over_the_oracle_unet_matches_the_reference_apply_model(golden, case, tie):
    """tests/split_ref.py is what the GPU tests compare against: pinned here to the reference's apply_model outputs, at the
    tolerance test_oracle_golden.py uses for unet_t2a (2e-5 absolute)."""
    from oracle import unet as O_unet
    g = golden("split_apply")
    _, ks, stride = R.CASES[case]
    tag = case + ("_tie" if tie else "")
    x, t, c = (torch.from_numpy(g[k + "_" + tag]) for k in ("x", "t", "c"))
    sd = WT.make_unet_state_dict(C.UNET_T2A, seed=0)
    p = SP.plan(R.params(case, tie), x.shape[2], x.shape[3], down=2)
    with torch.no_grad():
        y = R.apply_model_split(lambda z, tt: O_unet.unet_forward(sd, C.UNET_T2A, z, tt, c), x, t, p.weight, ks, stride)
    err = np.abs(y.numpy() - g["y_" + tag].astype(np.float64)).max()
    assert err <= 2e-5, (tag, err)


def test_unfold_restatement_is_the_reference_view():
    """ddpm_audio.py:582-585: z.view(B, -1, kh, kw, L)[..., l] is crop l."""
    x = torch.arange(2 * 3 * 12 * 24, dtype=torch.float32).reshape(2, 3, 12, 24)
    z = R.unfold(x, (8, 16), (4, 8)).reshape(2, 4, 3, 8, 16)
    for l, (y0, x0) in enumerate([(0, 0), (0, 8), (4, 0), (4, 8)]):
        assert torch.equal(z[:, l], x[:, :, y0:y0 + 8, x0:x0 + 16])


def test_model_attribute_is_read_as_the_reference_reads_it():
    """hasattr(self, "split_input_params") (ddpm_audio.py:572), without building a model (no GPU here)."""
    from audiogpt_amd.ldm.latent_diffusion import LatentDiffusionAudio
    m = object.__new__(LatentDiffusionAudio)
    m.conditioning_key = "crossattn"
    assert m.split_params() is None
    m.split_input_params = R.params("A")
    assert m.split_params() is m.split_input_params
    m.conditioning_key = "concat"
    with pytest.raises(MaaError, match="concat"):
        m.split_params()


def test_samplers_hand_the_attribute_to_the_device_loops():
    from audiogpt_amd.ldm.ddim import DDIMSampler
    from audiogpt_amd.ldm.plms import PLMSSampler
    from audiogpt_amd.pipeline import alphas_cumprod_f32

    class U:
        def __init__(self):
            self.calls = []

        def _rec(self, name, x, kw):
            self.calls.append((name, kw.get("split")))
            return x.clone(), [], []

        def ddim_sample(self, x, *a, **kw):
            return self._rec("ddim", x, kw)

        def plms_sample(self, x, *a, **kw):
            return self._rec("plms", x, kw)

        def ddim_decode(self, x, *a, **kw):
            return self._rec("decode", x, kw)[0]

    class M:
        def __init__(self):
            ldm = C.LDM_T2A
            self.num_timesteps = ldm["timesteps"]
            self.alphas_cumprod = torch.from_numpy(alphas_cumprod_f32(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"]))
            self.device = torch.device("cpu")
            self.conditioning_key = "crossattn"
            self.unet = U()

    m = M()
    kw = dict(S=4, batch_size=1, shape=[4, 8, 40], conditioning=torch.zeros(1, 4, 1024), verbose=False)
    d = DDIMSampler(m)
    d.sample(**kw)
    PLMSSampler(m).sample(**kw)
    m.split_input_params = R.params("A")
    d.sample(**kw)
    d.decode(torch.zeros(1, 4, 8, 40), torch.zeros(1, 4, 1024), 2)
    PLMSSampler(m).sample(**kw)
    assert m.unet.calls == [("ddim", None), ("plms", None), ("ddim", m.split_input_params), ("decode", m.split_input_params),
                            ("plms", m.split_input_params)]


@pytest.fixture(scope="module")
def lib():
    from audiogpt_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _fake(n=1):
    return ctypes.c_void_p(16 * n)          # a non-null pointer that the argument checks never dereference


def test_new_entries_are_declared_bound_and_reject_bad_arguments(lib):
    from audiogpt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "maa.h")).read(), flags=re.S)
    for name in ("maa_unet_forward_split", "maa_op_unfold", "maa_op_fold"):
        assert name in _lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1)
        assert len(getattr(lib, name).argtypes) == len(decl.split(",")), name
    w = (ctypes.c_float * 4)()
    assert lib.maa_unet_forward_split(None, None, None, None, None, 1, 8, 40, 8, 16, 8, 8, None, None) < 0
    assert b"null pointer" in lib.maa_last_error()
    assert lib.maa_op_unfold(None, None, 1, 4, 8, 40, 8, 16, 8, 8, None) < 0
    assert b"null pointer" in lib.maa_last_error()
    assert lib.maa_op_fold(None, None, None, 1, 4, 8, 40, 8, 16, 8, 8, None) < 0
    assert b"null pointer" in lib.maa_last_error()
    # geometry the kernels do not cover, then a well-formed call reaching the (null) context
    assert lib.maa_op_unfold(None, _fake(1), 1, 4, 8, 40, 8, 16, 8, 16, _fake(2)) < 0
    assert b"in no crop" in lib.maa_last_error()
    assert lib.maa_op_fold(None, _fake(1), w, 1, 4, 8, 40, 16, 16, 8, 8, _fake(2)) < 0
    assert b"larger than the latent" in lib.maa_last_error()
    assert lib.maa_unet_forward_split(None, _fake(1), _fake(2), _fake(3), None, 1, 8, 40, 8, 16, 8, 8, w, _fake(4)) < 0
    assert b"null context" in lib.maa_last_error()
    assert lib.maa_op_unfold(None, _fake(1), 1, 4, 8, 40, 8, 16, 8, 8, _fake(2)) < 0
    assert b"null context" in lib.maa_last_error()
    # the argument structure carries the split fields at its end
    names = [f[0] for f in _lib.maa_ddim_args._fields_]
    assert names[-5:] == ["split_kh", "split_kw", "split_sh", "split_sw", "h_split_weight"]
    a = _lib.maa_ddim_args()
    assert (a.split_kh, a.split_kw, a.split_sh, a.split_sw) == (0, 0, 0, 0) and not a.h_split_weight
