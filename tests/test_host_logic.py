"""Host-side logic of the drop-in layer, checked on CPU (no GPU, no compute calls into the library):
schedules, weight folding, the vocoder registry, "no CPU fallback", and that the product never imports the oracle."""
import ast
import os

import numpy as np
import pytest
import torch

from audiogpt_amd import config as C
from audiogpt_amd import weights as WT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ldm", [C.LDM_T2A, C.LDM_INPAINT], ids=["t2a", "inpaint"])
@pytest.mark.parametrize("S", [10, 100, 4])
def test_ddim_schedule_matches_oracle(ldm, S):
    """pipeline.ddim_schedule (what the C loop is driven by) == the oracle's restatement of ddim.py:27-56 / util.py:46-74."""
    from audiogpt_amd.pipeline import alphas_cumprod_f32, ddim_schedule
    from oracle import ddim as O
    ac = alphas_cumprod_f32(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
    ac_o = O.alphas_cumprod(ldm["timesteps"], ldm["linear_start"], ldm["linear_end"])
    assert np.array_equal(ac, ac_o.numpy())
    steps, a, ap = ddim_schedule(S, ac)
    steps_o = O.ddim_timesteps(S, ldm["timesteps"])
    a_o, ap_o, sg, _ = O.ddim_tables(ac_o, steps_o)
    assert steps.tolist() == steps_o.tolist() and steps[0] == 1 and steps.max() < ldm["timesteps"]
    assert np.array_equal(a, a_o.numpy()) and np.array_equal(ap, ap_o.numpy())
    assert float(ap[0]) == float(ac[0])                       # a_prev[0] = alphas_cumprod[0], not 1 (util.py:63-69)
    assert float(sg.abs().max()) == 0.0                       # eta = 0


def test_fold_weight_norm_is_torch_remove_weight_norm():
    """weights.fold_weight_norm == torch.nn.utils.weight_norm's w = g * v / ||v|| for Conv1d and ConvTranspose1d."""
    g = torch.Generator().manual_seed(3)
    for mod in (torch.nn.Conv1d(6, 10, 5), torch.nn.ConvTranspose1d(6, 10, 4, stride=2)):
        m = torch.nn.utils.weight_norm(mod)
        with torch.no_grad():
            m.weight_g.copy_(torch.rand(m.weight_g.shape, generator=g) + 0.5)
            m.weight_v.copy_(torch.randn(m.weight_v.shape, generator=g))
        sd = {"c.weight_g": m.weight_g.detach().clone(), "c.weight_v": m.weight_v.detach().clone(),
              "c.bias": m.bias.detach().clone()}
        ref = torch.nn.utils.remove_weight_norm(m).weight.detach()
        out = WT.fold_weight_norm(sd)
        assert set(out) == {"c.weight", "c.bias"}
        assert torch.allclose(out["c.weight"], ref, rtol=1e-6, atol=1e-7)


def test_strip_prefix_selects_submodule():
    sd = {"model.diffusion_model.a.weight": 1, "first_stage_model.b": 2, "scale_factor": 3}
    assert WT.strip_prefix(sd, "model.diffusion_model.") == {"a.weight": 1}


def test_vocoder_registry_mirrors_reference():
    """NeuralSeq/vocoders/base_vocoder.py:1-19: registered short name, class name, or dotted path."""
    from audiogpt_amd.vocoder import hifigan as V
    assert V.get_vocoder_cls({"vocoder": "HifiGAN"}) is V.HifiGAN
    assert V.get_vocoder_cls({"vocoder": "hifigan"}) is V.HifiGAN
    assert V.get_vocoder_cls({"vocoder": "audiogpt_amd.vocoder.hifigan.HifiGAN"}) is V.HifiGAN

    @V.register_vocoder
    class Dummy(V.BaseVocoder):
        pass
    assert V.get_vocoder_cls({"vocoder": "dummy"}) is Dummy


def test_no_cpu_fallback():
    """Without a GPU every product entry point raises: tools, pipeline and vocoders build a backend.Context first."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from audiogpt_amd import _lib
    from audiogpt_amd.pipeline import MakeAnAudio
    from audiogpt_amd.tools import T2A
    from audiogpt_amd.vocoder.hifigan import HifiGanGenerator
    for make in (lambda: MakeAnAudio("cuda:0"), lambda: T2A("cuda:0"),
                 lambda: HifiGanGenerator(dict(C.HIFIGAN_NS_128), device="cuda:0")):
        with pytest.raises((_lib.MaaError, AssertionError, RuntimeError)):
            make()


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under audiogpt_amd/ may import it (statically checked)."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "audiogpt_amd")):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            tree = ast.parse(open(path).read(), path)
            for node in ast.walk(tree):
                names = []
                if isinstance(node, ast.Import):
                    names = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom):
                    names = [node.module or ""]
                if any(n == "oracle" or n.startswith("oracle.") for n in names):
                    bad.append(path)
    assert not bad, bad


def test_unet_layer_plan_matches_survey_counts():
    """weights.unet_layers(T2A) reproduces the block map of SURVEY 8a/U1: 12 ResBlocks, 11 SpatialTransformers."""
    layers = WT.unet_layers(C.UNET_T2A)
    flat = []

    def walk(x):
        if isinstance(x, dict):
            if "kind" in x:
                flat.append(x["kind"])
            for v in x.values():
                walk(v)
        elif isinstance(x, (list, tuple)):
            for v in x:
                walk(v)
    walk(layers)
    if flat:                                                   # plan exposes per-layer kinds
        kinds = [str(k).lower() for k in flat]
        assert sum("res" in k for k in kinds) == 12
        assert sum(("st" == k) or ("transformer" in k) or ("spatial" in k) for k in kinds) == 11
    sd = WT.make_unet_state_dict(C.UNET_T2A, seed=0)
    n_params = sum(int(np.prod(v.shape)) for v in sd.values())
    assert abs(n_params - 160.22e6) < 0.05e6                   # 160.2 M parameters


def test_pmc_traffic_derivation_and_staleness_guard(tmp_path):
    """scripts/pmc_traffic_json.py on a synthetic PMC summary: FETCH_SIZE doubled (gfx950 counts 128-B requests as 64 B),
    KB -> bytes, a split-K contraction = its GEMM launches + its reduce launches, per-step launch counts and the source hash
    that bench.py uses to refuse numbers taken on another binary."""
    import json
    import subprocess
    import sys

    from audiogpt_amd.build import _source_hash
    txt = tmp_path / "pmc.txt"
    txt.write_text(
        "== FETCH_SIZE GRBM_GUI_ACTIVE  (4 DDIM steps)\n"
        "igemm_dma_kernel<64, 64, 2, 2, 4>                  grid 249600    launches   200  FETCH_SIZE=1000000  GRBM_GUI_ACTIVE=1\n"
        "igemm_dma_kernel<64, 64, 2, 2, 4>                  grid 125440    launches    64  FETCH_SIZE=320000  GRBM_GUI_ACTIVE=1\n"
        "igemm_dma2_kernel<128, 128, 2, 2, 4, true, 0>      grid 64000     launches    40  FETCH_SIZE=400000  GRBM_GUI_ACTIVE=1\n"
        "splitk_reduce_kernel<1>                            grid 128000    launches    40  FETCH_SIZE=200000  GRBM_GUI_ACTIVE=1\n"
        "== WRITE_SIZE GRBM_GUI_ACTIVE  (4 DDIM steps)\n"
        "igemm_dma_kernel<64, 64, 2, 2, 4>                  grid 249600    launches   200  WRITE_SIZE=500000  GRBM_GUI_ACTIVE=1\n"
        "igemm_dma_kernel<64, 64, 2, 2, 4>                  grid 125440    launches    64  WRITE_SIZE=100000  GRBM_GUI_ACTIVE=1\n"
        "igemm_dma2_kernel<128, 128, 2, 2, 4, true, 0>      grid 64000     launches    40  WRITE_SIZE=640000  GRBM_GUI_ACTIVE=1\n"
        "splitk_reduce_kernel<1>                            grid 128000    launches    40  WRITE_SIZE=160000  GRBM_GUI_ACTIVE=1\n")
    out = str(tmp_path / "t.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pmc_traffic_json.py"), str(txt), "bf16x3", "4", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    t = json.load(open(out))
    assert t["precision"] == "bf16x3" and t["source_hash"] == _source_hash() and t["ddim_steps"] == 4
    k = t["kernels"]["igemm_dma_bf16x3<64x64>"]
    assert k["launches"] == 264 and k["launches_per_ddim_step"] == 66.0
    assert abs(k["hbm_bytes_per_launch"] - (2 * 1320000 + 600000) * 1024.0 / 264) < 1e-6
    k2 = t["kernels"]["igemm_dma2_bf16x3<128x128,splitK>"]
    assert k2["launches"] == 40 and abs(k2["hbm_bytes_per_launch"] - (2 * 600000 + 800000) * 1024.0 / 40) < 1e-6


def test_bench_line_contract_of_a_gpu_run():
    """A bench line measured on the MI355X this round (profiles/r3/r3_bf16x3_bench.json, written by scripts/gpu_profile.sh)
    carries every field of the driver's contract plus roofline, cpu_baseline and the secondary workloads, states its method
    in the metric string, and its arithmetic is self-consistent."""
    import json
    path = os.path.join(ROOT, "profiles", "r3", "r3_bf16x3_bench.json")
    if not os.path.exists(path):
        import pytest
        pytest.skip("no round-3 bench line committed yet")
    d = json.load(open(path))
    assert "batches of 8 prompts in flight per GPU" in d["metric"] and d["config"]["batches_in_flight"] == 3
    assert d["one_batch_in_flight"]["value"] > 0 and d["batch_latency_ms"]["in_flight"] > d["batch_latency_ms"]["alone"] > 0
    for w in ("hifigan64", "mixed"):
        sec = d["secondary"][w]
        assert sec["value"] > 0 and sec["cpu_baseline"]["value"] > 0 and 0 < sec["roofline"]["frac"] < 1
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["vs_baseline"] is None and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0
    assert abs(d["value"] - d["config"]["audio_seconds_per_step"] / (d["ms_per_step"] / 1e3)) < 1e-6 * d["value"]


def test_bench_box_sampler_reads_amdgpu_sysfs(tmp_path):
    """bench.BoxSampler (clock / power of the box during the timed region) against a fake sysfs tree, and on a machine with
    no such tree (this container): it never raises and reports None."""
    import sys
    import time
    sys.path.insert(0, ROOT)
    import bench
    assert bench.BoxSampler.parse_sclk("0: 132Mhz\n1: 2242Mhz *\n") == 2242
    assert bench.BoxSampler.parse_sclk("S: 95Mhz *") == 95 and bench.BoxSampler.parse_sclk("0: 132Mhz\n") is None
    dev = tmp_path / "card0" / "device"
    (dev / "hwmon" / "hwmon3").mkdir(parents=True)
    (dev / "pp_dpm_sclk").write_text("0: 132Mhz\n1: 2230Mhz *\n")
    (dev / "pp_dpm_mclk").write_text("0: 900Mhz\n1: 2000Mhz *\n")
    (dev / "pp_dpm_fclk").write_text("0: 1200Mhz\n1: 1800Mhz *\n")      # (no pp_dpm_socclk: reported as None)
    (dev / "hwmon" / "hwmon3" / "power1_average").write_text("1350000000\n")
    with bench.BoxSampler(root=str(tmp_path), period=0.02) as sm:
        time.sleep(0.2)
    r = sm.summary()
    assert r["sclk_mhz_median"] == 2230 and r["sclk_mhz_min"] == 2230 and abs(r["socket_power_w_median"] - 1350.0) < 1e-6 and r["samples"] >= 2
    assert r["mclk_mhz_median"] == 2000 and r["fclk_mhz_median"] == 1800 and r["socclk_mhz_median"] is None
    with bench.BoxSampler(root=str(tmp_path / "nothing")) as sm:
        pass
    assert sm.summary()["sclk_mhz_median"] is None and sm.summary()["samples"] == 0
    assert r["matched_by"].startswith("first_amdgpu_card") and r["pci_bus_id"] is None


def test_bench_box_sampler_follows_the_hip_devices_pci_address(tmp_path, monkeypatch):
    """On a multi-GPU host the sampled card must be the HIP device's own: a fake PCI tree with two cards, the second one ours
    (the first card with pp_dpm_sclk was sampled whatever device the benchmark ran on)."""
    import sys
    import time
    sys.path.insert(0, ROOT)
    import bench
    pci = tmp_path / "pci"
    for bdf, mhz, uw in (("0000:05:00.0", 132, 90000000), ("0000:85:00.0", 2210, 1380000000)):
        d = pci / bdf
        (d / "hwmon" / "hwmon7").mkdir(parents=True)
        (d / "pp_dpm_sclk").write_text("0: 132Mhz%s\n1: %dMhz%s\n" % (" *" if mhz == 132 else "", max(mhz, 133), " *" if mhz != 132 else ""))
        (d / "hwmon" / "hwmon7" / "power1_average").write_text("%d\n" % uw)
    monkeypatch.setattr(bench.BoxSampler, "pci_bdf", staticmethod(lambda device: "0000:85:00.0"))
    with bench.BoxSampler(device="cuda:1", root=str(tmp_path / "nodrm"), pci_root=str(pci), period=0.02) as sm:
        time.sleep(0.15)
    r = sm.summary()
    assert r["pci_bus_id"] == "0000:85:00.0" and r["matched_by"] == "pci_bus_id"
    assert r["sclk_mhz_median"] == 2210 and abs(r["socket_power_w_median"] - 1380.0) < 1e-6
    # the address as torch reports it: three integers -> dddd:bb:dd.f
    class P:
        pci_domain_id, pci_bus_id, pci_device_id = 0, 0x85, 0
    monkeypatch.undo()
    import torch
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda d: P())
    assert bench.BoxSampler.pci_bdf("cuda:1") == "0000:85:00.0"


def test_mel_front_end_restatement():
    """audiogpt_amd/mel.py restates librosa's stft / mel filter bank (absent here: parity unpinned, see its docstring).
    Checked against an independent framing (scipy.signal.stft on the explicitly padded signal), the filter bank's
    defining properties, an analytic tone, and the TRANSFORMS_16000 level mapping."""
    import numpy as np
    import scipy.signal as ss

    from audiogpt_amd import mel as M
    fb = M.mel_filterbank()
    assert fb.shape == (80, 513) and fb.dtype == np.float32 and (fb >= 0).all()
    freqs = np.linspace(0, 8000, 513)
    centres = (fb * freqs[None]).sum(1) / fb.sum(1)
    assert (np.diff(centres) > 0).all() and 125 < centres[0] < 200 and 7000 < centres[-1] < 7600
    assert fb[:, freqs < 125].sum() == 0 and fb[:, freqs > 7600].sum() == 0
    # Slaney normalisation: every filter integrates to ~1 over frequency (bin width 15.625 Hz)
    area = fb.sum(1) * (8000 / 512)
    assert np.allclose(area, 1.0, atol=0.15), (area.min(), area.max())
    rs = np.random.RandomState(0)
    x = rs.randn(4 * 16000).astype(np.float32) * 0.1
    for mode in ("constant", "reflect"):
        S = M.stft_magnitude(x, pad_mode=mode)
        assert S.shape == (513, 1 + len(x) // 256)
        xp = np.pad(x, 512, mode=mode)
        _, _, Z = ss.stft(xp, window="hann", nperseg=1024, noverlap=768, boundary=None, padded=False)
        ref = np.abs(Z) * ss.get_window("hann", 1024).sum()
        assert np.abs(ref - S).max() <= 1e-5 * S.max()
    t = np.arange(848 * 256) / 16000.0
    tone = (0.5 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    m = M.transforms_16000(tone)
    assert m.shape == (80, 849) and m.min() >= 0 and m.max() <= 1
    k = int(m[:, 400].argmax())
    assert abs(centres[k] - 1000.0) < 60
    assert M.transforms_16000(np.zeros(20000, dtype=np.float32)).max() == 0.0        # silence: 20 log10(1e-5) + 80 < 0 -> 0
    sr, wav = 16000, (tone[:5 * 16000] * 32767).astype(np.int16)
    assert M.gen_mel_audio((sr, wav)).shape == (80, 1 + (5 * 16000 + 848 * 256) // 256)   # short input: reference's full-clip pad
    assert M.gen_mel_audio((sr, np.stack([wav, wav], 1))).shape[0] == 80                 # stereo -> mono
    assert M.gen_mel_audio((32000, np.repeat(wav, 2))).shape[0] == 80                    # resampled to 16 kHz


def test_mel_front_end_against_the_transformers_restatement_of_librosa():
    """librosa is absent; `transformers.audio_utils` ships its own implementation of the two librosa routines the
    front end uses (Slaney-scale, Slaney-normalised triangular mel filters; centred Hann STFT).  Two independent
    restatements of the same published algorithm agreeing to rounding is the strongest pin this image allows."""
    import numpy as np
    au = pytest.importorskip("transformers.audio_utils")
    from audiogpt_amd import mel as M
    fb = au.mel_filter_bank(num_frequency_bins=1 + M.N_FFT // 2, num_mel_filters=M.N_MELS, min_frequency=M.FMIN,
                            max_frequency=M.FMAX, sampling_rate=M.SAMPLE_RATE, norm="slaney", mel_scale="slaney")
    assert np.abs(fb.T - M.mel_filterbank()).max() < 1e-8
    x = (np.random.RandomState(0).randn(2 * M.SAMPLE_RATE) * 0.1).astype(np.float32)
    win = au.window_function(M.N_FFT, "hann", periodic=True)
    for pad_mode in ("constant", "reflect"):
        s = au.spectrogram(x, win, frame_length=M.N_FFT, hop_length=M.HOP, fft_length=M.N_FFT, power=1.0, center=True,
                           pad_mode=pad_mode)
        m = M.stft_magnitude(x, pad_mode=pad_mode)
        assert s.shape == m.shape and np.abs(s - m).max() < 1e-5 * np.abs(m).max()


def test_scorer_front_end_tables():
    """Host-built constants of the device front ends: the windowed DFT basis against numpy's FFT and
    torch.stft, the 44.1 kHz filter bank against transformers.audio_utils, torchaudio's resampling kernel bank by its
    defining properties (torchaudio is absent: unpinned), and the default STFT padding."""
    import numpy as np
    import torch
    from scipy.signal import get_window

    from audiogpt_amd import config as C
    from audiogpt_amd import mel as M
    from audiogpt_amd.clap import sinc_resample_kernel
    assert M.PAD_MODE == os.environ.get("AUDIOGPT_AMD_STFT_PAD", "reflect")          # librosa 0.9.x, the reference's
    basis = M.dft_basis(1024)
    assert basis.shape == (1026, 1024) and basis.dtype == np.float32
    x = np.random.RandomState(0).randn(3000).astype(np.float32)
    F = np.fft.rfft(x[:1024] * get_window("hann", 1024, fftbins=True))
    y = basis.astype(np.float64) @ x[:1024]
    assert np.abs(y[:513] - F.real).max() < 1e-5 and np.abs(y[513:] - F.imag).max() < 1e-5
    # the framed-GEMM formulation == torch.stft (centre, reflect), power spectrogram
    xt = torch.from_numpy(x)[None]
    st = torch.stft(xt, 1024, hop_length=320, window=torch.hann_window(1024, periodic=True), center=True, pad_mode="reflect",
                    return_complex=True)
    fr = torch.nn.functional.pad(xt[:, None], (512, 512), mode="reflect")[:, 0].unfold(1, 1024, 320)
    Y = fr.double() @ torch.from_numpy(basis).double().T
    P = (Y[..., :513] ** 2 + Y[..., 513:] ** 2)[0].T
    ref = (st.real ** 2 + st.imag ** 2)[0].double()
    assert P.shape == ref.shape == (513, 1 + 3000 // 320) and float((P - ref).abs().max()) < 1e-4 * float(ref.max())
    a = C.CLAP_SCORER
    au = pytest.importorskip("transformers.audio_utils")
    fb = au.mel_filter_bank(num_frequency_bins=513, num_mel_filters=a["mel_bins"], min_frequency=a["fmin"], max_frequency=a["fmax"],
                            sampling_rate=a["sampling_rate"], norm="slaney", mel_scale="slaney")
    mine = M.mel_filterbank(sr=a["sampling_rate"], n_fft=1024, n_mels=a["mel_bins"], fmin=a["fmin"], fmax=a["fmax"])
    assert np.abs(fb.T - mine).max() < 1e-8
    # resampler: 16 k -> 44.1 k reduces to 160 -> 441; phase 0 is (nearly) the identity tap; every phase has DC gain ~1;
    # a 1 kHz tone comes out as a 1 kHz tone of the same amplitude
    k, width = sinc_resample_kernel(16000, 44100)
    assert k.shape == (441, 2 * width + 160) and width == 7
    assert abs(k[0, width] - 0.99) < 1e-6 and np.abs(k.sum(1) - 1.0).max() < 2e-3
    t = np.arange(16000) / 16000.0
    tone = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
    xp = np.pad(tone, (width, width + 160))
    frames = np.lib.stride_tricks.sliding_window_view(xp, k.shape[1])[::160]
    out = (frames @ k.T).reshape(-1)[:44100]
    want = np.sin(2 * np.pi * 1000.0 * np.arange(44100) / 44100.0)
    assert np.abs(out[2000:42000] - want[2000:42000]).max() < 5e-3


def test_resampler_matches_an_independent_polyphase_implementation():
    """torchaudio is absent, so its default resampler (CLAPWrapper.py:103-110: T.Resample(16000 -> 44100), sinc interpolation with a
    Hann window, lowpass_filter_width 6, rolloff 0.99) cannot be run here.  Its restatements -- the oracle's strided convolution
    and the kernel bank the device contraction uses -- are pinned to an INDEPENDENT second implementation instead: scipy's polyphase
    engine (resample_poly / upfirdn) given the same documented prototype FIR sampled on the 1 / (orig * new) grid.  Zero padding at
    both ends and the output length ceil(new n / orig) are the same in both (tests/golden/manifest.json, _third_party_pins)."""
    import math

    import numpy as np
    import torch
    from scipy.signal import resample_poly

    from audiogpt_amd.clap import sinc_resample_kernel
    from oracle import clap_audio as O
    for orig_f, new_f, n in ((16000, 44100, 5000), (22050, 44100, 3001), (48000, 44100, 4097)):
        lpw, rolloff = 6, 0.99
        g = math.gcd(orig_f, new_f)
        orig, new = orig_f // g, new_f // g
        base = min(orig, new) * rolloff
        half = int(math.ceil(lpw * orig * new / base))
        t = np.clip(np.arange(-half, half + 1, dtype=np.float64) * base / (orig * new), -lpw, lpw)
        with np.errstate(divide="ignore", invalid="ignore"):
            proto = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t)) * np.cos(t * np.pi / lpw / 2) ** 2 * (base / orig)
        x = np.random.RandomState(n).randn(2, n)
        want = resample_poly(x, new, orig, axis=-1, window=proto / new)          # (scipy multiplies its taps by `up`)
        got = O.resample(torch.from_numpy(x).float(), orig_f, new_f).numpy()
        assert got.shape == want.shape == (2, math.ceil(new * n / orig))
        assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max(), (orig_f, np.abs(got - want).max())
        # the device path's kernel bank, applied as the strided contraction the library runs
        k, width = sinc_resample_kernel(orig_f, new_f)
        xp = np.pad(x[0].astype(np.float32), (width, width + orig))
        frames = np.lib.stride_tricks.sliding_window_view(xp, k.shape[1])[::orig]
        dev = (frames.astype(np.float64) @ k.T.astype(np.float64)).reshape(-1)[:want.shape[1]]
        assert np.abs(dev - want[0]).max() <= 2e-6 * np.abs(want).max()


def test_product_tree_never_touches_the_oracle_or_the_reference_tree():
    """The oracle is test infrastructure: nothing under audiogpt_amd/ (or include/) may import or name it, and nothing
    that runs on the GPU box (product, bench.py, __graft_entry__.py, tests other than the golden generator) may read
    the reference tree."""
    import re
    REF = "/root/" + "reference"          # (spelled in two pieces: this file is scanned too)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    product = []
    for base, _, files in os.walk(os.path.join(root, "audiogpt_amd")):
        if "_build" in base or "__pycache__" in base:
            continue
        product += [os.path.join(base, f) for f in files if f.endswith((".py", ".cpp", ".hip", ".h"))]
    assert len(product) > 30
    imp = re.compile(r"^\s*(from|import)\s+oracle\b|[\"']oracle[/\"']", re.M)
    for path in product:
        text = open(path, encoding="utf-8").read()
        assert not imp.search(text), path + " refers to the oracle"
        assert REF not in text, path + " names the reference tree"
    runtime = [os.path.join(root, f) for f in ("bench.py", "__graft_entry__.py")]
    runtime += [os.path.join(root, "tests", f) for f in os.listdir(os.path.join(root, "tests")) if f.endswith(".py")]
    for path in runtime:
        assert REF not in open(path, encoding="utf-8").read(), path + " would need the reference tree at run time"


def test_pmc_traffic_tables_keep_their_own_source_stamp(tmp_path):
    """scripts/pmc_traffic_json.py (profiles/pmc_traffic.json, what bench.py's `roofline.traffic` reads): the secondary
    workloads' tables are stamped one by one, a primary pass keeps the sections measured on the same sources whatever the
    file's older top-level stamp says (round 4: the sections were dropped because the file still carried round 3's hash), and
    drops a section measured on other sources."""
    import json
    import subprocess
    import sys
    from audiogpt_amd.build import _source_hash
    prof = os.path.join(ROOT, "profiles", "r4")
    out = tmp_path / "pmc_traffic.json"
    out.write_text(json.dumps({"precision": "bf16x3", "source_hash": "0" * 64, "ddim_steps": 4, "kernels": {}}))   # an older round's file
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pmc_traffic_json.py"), *a], check=True,
                                    capture_output=True, timeout=120)
    run(os.path.join(prof, "r4_hifigan64_pmc_fetch_write.txt"), "bf16x3", "1", str(out), "--section", "hifigan64")
    run(os.path.join(prof, "r4_mixed_pmc_fetch_write.txt"), "bf16x3", "4", str(out), "--section", "mixed")
    d = json.loads(out.read_text())
    assert set(d["secondary"]) == {"hifigan64", "mixed"} and d["secondary"]["mixed"]["source_hash"] == _source_hash()
    d["secondary"]["mixed"]["source_hash"] = "1" * 64          # pretend this one was taken on other sources
    out.write_text(json.dumps(d))
    run(os.path.join(prof, "r4_bf16x3_pmc_fetch_write.txt"), "bf16x3", "4", str(out))
    d = json.loads(out.read_text())
    assert d["source_hash"] == _source_hash() and set(d.get("secondary", {})) == {"hifigan64"}
    e = d["kernels"]["igemm_pp_bf16x3<256x160,splitK>"]
    assert e["launches_per_ddim_step"] == 24.0 and 1.2e8 < e["hbm_bytes_per_launch"] < 1.6e8 and 0.3 < e["mfma_busy"] < 0.6
    k = d["secondary"]["hifigan64"]["kernels"]["igemm_pp_bf16x3<256x128>"]
    assert k["launches_per_unit"] == 36.0 and k["hbm_bytes_per_launch"] > 4e9


def test_bench_stdout_line_fits_the_drivers_capture(capsys):
    """the driver keeps the last 8.6 kB of stdout, so the ONE JSON line must stay under 6 kB and still carry,
    per workload, value / ms_per_step / roofline{kernel, frac, achieved, traffic, mfma_busy, avg_launch_us} / cpu_baseline /
    parity, plus one_batch_in_flight, one_batch_two_streams and box.calib at the top level.  Checked on the largest full record
    committed (round 4's 17 kB line) and on bench.main's own stub path."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r4", "r4_bf16x3_bench.json")))
    # worst case: every workload with every attachment, long kernel names, traffic on every roofline
    for w in full["secondary"].values():
        if "roofline" in w:
            w["roofline"].setdefault("traffic", 123456789.0)
            w["roofline"]["traffic"] = w["roofline"]["traffic"] or 123456789.0
            w["roofline"]["mfma_busy"] = 0.123456
            w["roofline"]["traffic_source"] = "profiles/pmc_traffic.json"
    full["box"]["class"] = "slow(l2_read_gbs,infinity_cache_read_gbs)"
    line = bench.slim_line(full, "gpurun_out/bench_detail.json")
    assert len(line) <= bench.LINE_LIMIT == 6144 and "\n" not in line
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "one_batch_in_flight", "one_batch_two_streams", "box"):      # (round 4 record: the two-stream experiment of that round)
        assert k in d, k
    assert d["value"] == pytest.approx(full["value"], rel=1e-6) and d["config"]["batches_in_flight"] == 3
    assert d["one_batch_in_flight"]["value"] == pytest.approx(full["one_batch_in_flight"]["value"], rel=1e-4)
    assert set(d["box"]["calib"]) >= {"mfma_bf16_tflops", "copy_gbs", "l2_read_gbs", "infinity_cache_read_gbs"}
    r = d["roofline"]
    assert r["kernel"] and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4 and r["traffic"] > 0 and r["avg_launch_us"] > 0
    assert "kernel_time_ms" not in r and "traffic_note" not in r
    assert set(d["secondary"]) == {"hifigan64", "mixed", "t2a_bf16", "t2a_bigvgan", "tool_latency"}
    for name, w in d["secondary"].items():
        assert w["value"] > 0 and w["cpu_baseline"]["value"] > 0 and w["cpu_baseline"]["kind"] == "port", name
        assert 0 < w["roofline"]["frac"] < 1 and w["roofline"]["kernel"] and w["roofline"]["traffic"] > 0, name
    assert d["secondary"]["t2a_bf16"]["parity"]["meets_gate"] is False and d["secondary"]["t2a_bigvgan"]["parity"]["meets_gate"] is True
    assert d["secondary"]["t2a_bf16"]["one_batch_in_flight"]["value"] > 0
    # the stub path of main() prints exactly one line, through the same function
    bench.main(["--stub-cpu", "--full", "--steps", "2", "--warmup", "1", "--inflight", "2"])
    out = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(out) == 1 and len(out[0]) <= bench.LINE_LIMIT
    assert json.loads(out[0])["detail"].endswith("bench_detail.json")


def test_bench_plain_run_and_dump_outputs(tmp_path, capsys):
    """A plain run (no --full) prints the contract line only -- no detail file, no hash -- and --dump-outputs writes the last
    timed step's arrays as float32 .npy files, the same ones on every run with the same arguments."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        bench.main(["--stub-cpu", "--steps", "3", "--warmup", "1", "--inflight", "2", "--dump-outputs", str(d)])
        out = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
        dumps.append({p.name: np.load(str(p)) for p in d.iterdir()})
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and "detail" not in line and "wav_sha16" not in line
    assert set(dumps[0]) == {"waveform.npy"}      # (the stub pipeline makes no mel / latent)
    w = dumps[0]["waveform.npy"]
    assert w.dtype == np.float32 and w.shape == (8, 64) and np.isfinite(w).all()
    assert np.array_equal(w, dumps[1]["waveform.npy"])


def test_box_class_thresholds():
    """bench.box_class: a box whose L2 / Infinity-Cache reads fall under 85 % of the fast-class figures is labelled slow."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    fast = {"mfma_bf16_tflops": 2290.4, "copy_gbs": 5195.1, "l2_read_gbs": 23413.0, "infinity_cache_read_gbs": 6604.3}
    assert bench.box_class(fast) == "fast"
    assert bench.box_class(dict(fast, l2_read_gbs=15000.0)) == "slow(l2_read_gbs)"
    assert bench.box_class(dict(fast, infinity_cache_read_gbs=4000.0, l2_read_gbs=1.0)) == "slow(l2_read_gbs,infinity_cache_read_gbs)"
    assert bench.box_class({"error": "x"}) is None and bench.box_class(None) is None


def test_committed_traffic_table_carries_the_headlines_launch_mix(tmp_path):
    """What the round-5 validation tripped over: the counter passes had run with the library's default two CFG lanes (48 half-size
    convolutions per DDIM step) while bench.py's roofline pass runs a CFG step on one stream (24), so attach_traffic refused the
    table and the line said `traffic: null`.  The committed table must carry the dominant kernel at the headline's 24 launches per
    step and the profile scripts must ask for the headline's arrangement; bench.attach_traffic accepts a table only for the
    sources it was measured on (hash), the same precision and launch mix.  A committed table that is STALE against the current
    sources is a warning here, not a failure (CPU CI must not depend on a rocprofv3 pass on an MI355X) -- bench.py
    then reports `traffic: null` with a note, and scripts/gpu_profile.sh re-stamps the table."""
    import json
    import sys
    import warnings
    sys.path.insert(0, ROOT)
    import bench
    from audiogpt_amd.build import _source_hash
    t = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    if t["source_hash"] != _source_hash():
        warnings.warn("profiles/pmc_traffic.json was measured on other sources: re-run scripts/gpu_profile.sh on an MI355X "
                      "(bench.py reports traffic: null until then)")
    name = next(k for k in t["kernels"] if k.startswith("igemm_pp_bf16x3<256x160"))
    e = t["kernels"][name]
    assert e["launches_per_ddim_step"] == 24.0 and e["hbm_bytes_per_launch"] > 0 and 0 < e["mfma_busy"] < 1
    # the acceptance logic, on a copy of the table stamped with the current sources
    fresh = str(tmp_path / "pmc_traffic.json")
    t2 = json.loads(json.dumps(t))
    t2["source_hash"] = _source_hash()
    json.dump(t2, open(fresh, "w"))
    roof = {"kernel": name, "launches": 2400, "traffic": None}
    bench.attach_traffic(roof, "bf16x3", None, 100, table_path=fresh)
    assert roof["traffic"] == e["hbm_bytes_per_launch"] and roof["mfma_busy"] == e["mfma_busy"] and "NOT measured in this run" in roof["traffic_note"]
    # ... refused for the two-lane arrangement's launch count, and for sources other than the table's
    lanes = {"kernel": name, "launches": 4800, "traffic": None}
    bench.attach_traffic(lanes, "bf16x3", None, 100, table_path=fresh)
    assert lanes["traffic"] is None and "does not match" in lanes["traffic_note"]
    t2["source_hash"] = "0" * 64
    json.dump(t2, open(fresh, "w"))
    stale = {"kernel": name, "launches": 2400, "traffic": None}
    bench.attach_traffic(stale, "bf16x3", None, 100, table_path=fresh)
    assert stale["traffic"] is None and "does not match" in stale["traffic_note"]
    assert "set_cfg_split(False)" in open(os.path.join(ROOT, "scripts", "pmc_workload.py")).read()
    assert "--inflight 1 --cfg-split 0" in open(os.path.join(ROOT, "scripts", "gpu_profile.sh")).read()
    sec = t.get("secondary", {}).get("hifigan64")
    assert sec and sec["kernels"]["igemm_pp_bf16x3<256x128>"]["launches_per_unit"] == 36.0


def test_round5_record_slims_to_the_committed_line():
    """The full record of the round-5 validation run (profiles/r5/r5_bf16x3_bench_detail.json) -> the stdout line: within the limit,
    the literal configs[1] number (one batch owning the GPU, both CFG forms, bit-identical), box.class and every secondary value."""
    import json
    import sys
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r5", "r5_bf16x3_bench_detail.json")))
    line = bench.slim_line(full, "gpurun_out/bench_detail.json")
    assert len(line) <= bench.LINE_LIMIT
    d = json.loads(line)
    shipped = json.load(open(os.path.join(ROOT, "profiles", "r5", "r5_bf16x3_bench.json")))
    assert d["value"] == shipped["value"] and d["one_batch_in_flight"] == shipped["one_batch_in_flight"]
    assert d["one_batch_in_flight"]["cfg_lanes"] == 2 and d["one_batch_other_form"]["cfg_lanes"] == 1 and d["one_batch_other_form"]["bit_identical"] is True
    assert d["box"]["class"] == "fast" and d["config"]["cfg_lanes"] == 1 and d["config"]["batches_in_flight"] == 3
    assert {k: v["value"] for k, v in d["secondary"].items()} == {k: v["value"] for k, v in shipped["secondary"].items()}
    assert d["secondary"]["t2a_bf16"]["roofline"]["kernel"].startswith("igemm_dma_bf16<")      # the shipped engines' one-product form


def test_agent_tool_registration_resolves_on_the_drop_in_classes():
    """The agent builds `Tool(name=..., func=self.<tool>.<method>)` for the three Make-An-Audio classes
    (audio-chatgpt.py:1084 / :1154 T2A.inference, :1114 I2A.inference, :1120 Inpaint.show_mel_fn) and its Gradio callback calls
    `self.inpaint.inference(audio, image)` (:1355).  With INTEGRATION.md's import swap every one of those attribute look-ups
    must resolve on `audiogpt_amd.tools` with the reference's parameter names (no GPU: instances are made without __init__,
    exactly what attribute resolution at `init_tools` time needs)."""
    import inspect

    from audiogpt_amd import tools as T

    class Tool:                                   # the three fields init_tools passes to langchain's Tool
        def __init__(self, name, func, description):
            assert callable(func) and isinstance(name, str) and isinstance(description, str)
            self.name, self.func, self.description = name, func, description

    class Bot:
        t2a = object.__new__(T.T2A)
        i2a = object.__new__(T.I2A)
        inpaint = object.__new__(T.Inpaint)
    self = Bot()
    tools = [
        Tool(name="Generate Audio From User Input Text", func=self.t2a.inference, description="... a string ..."),
        Tool(name="Generate Audio From The Image", func=self.i2a.inference, description="... the image_path ..."),
        Tool(name="Audio Inpainting", func=self.inpaint.show_mel_fn, description="... the audio_path ..."),
    ]
    assert [t.func.__name__ for t in tools] == ["inference", "inference", "show_mel_fn"]
    callback = self.inpaint.inference                                                     # audio-chatgpt.py:1355
    # the reference's signatures (audio-chatgpt.py:201, 262, 452, 468, 492, 500, 529, 439), parameter for parameter
    want = {
        (T.T2A, "txt2audio"): ["text", "seed", "scale", "ddim_steps", "n_samples", "W", "H"],
        (T.T2A, "select_best_audio"): ["prompt", "wav_list"],
        (T.T2A, "inference"): ["text", "seed", "scale", "ddim_steps", "n_samples", "W", "H"],
        (T.I2A, "img2audio"): ["image", "seed", "scale", "ddim_steps", "W", "H"],
        (T.I2A, "inference"): ["image", "seed", "scale", "ddim_steps", "W", "H"],
        (T.Inpaint, "make_batch_sd"): ["mel", "mask", "num_samples"],
        (T.Inpaint, "gen_mel"): ["input_audio_path"],
        (T.Inpaint, "gen_mel_audio"): ["input_audio"],
        (T.Inpaint, "show_mel_fn"): ["input_audio_path"],
        (T.Inpaint, "inpaint"): ["batch", "seed", "ddim_steps", "num_samples", "W", "H"],
        (T.Inpaint, "inference"): ["input_audio", "mel_and_mask", "seed", "ddim_steps"],
    }
    for (cls, name), params in want.items():
        assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == params, (cls.__name__, name)
    assert inspect.signature(callback).parameters["seed"].default == 55
    # `self.cmap_transform = matplotlib.cm.viridis` (audio-chatgpt.py:424) is set by the constructor
    src = inspect.getsource(T.Inpaint.__init__)
    assert "self.cmap_transform = matplotlib.cm.viridis" in src


def test_librosa_resample_restatement_bank_equals_the_time_register_loop():
    """`Inpaint.gen_mel` resamples with librosa.resample = resampy "kaiser_best" (audio-chatgpt.py:462; both packages absent:
    unpinned).  The product runs it as a polyphase bank (mel.resampy_kernel_bank + the carry kernel, the device contraction's
    operands); oracle/resampy.py restates resampy's scalar loop with its running float64 time register.  The two must agree to
    fp32 rounding for down- and up-sampling, ratios with and without register drift, and lengths where int(n r) < ceil(n r)."""
    from audiogpt_amd import mel as M
    from oracle import resampy as R
    rs = np.random.RandomState(0)
    carried = 0
    for sr, n in ((44100, 30000), (8000, 9000), (48000, 20001), (22050, 15000), (32000, 7001), (11025, 9000), (44100, 441 * 40)):
        x = (rs.randn(n) * 0.1).astype(np.float32)
        want = R.librosa_resample(x, sr, 16000)
        got = M.librosa_resample(x, sr, 16000)
        assert want.dtype == got.dtype == np.float32 and want.shape == got.shape == (int(np.ceil(n * 16000 / sr)),)
        assert np.abs(want - got).max() <= 1e-6, (sr, np.abs(want - got).max())
        t = M.resampy_carries(int(n * 16000.0 / sr), sr, 16000)
        carried += t.size
        if int(n * (16000.0 / sr)) < want.shape[0]:
            assert want[-1] == 0 and got[-1] == 0                 # librosa.util.fix_length's zero sample
    assert carried > 50                                          # the 44.1 kHz family exercises the carry kernel
    assert M.resampy_carries(10 ** 5, 48000, 16000).size == 0    # 1 / ratio exact in binary: the register never drifts
    # without the carry kernel the bank alone is 1e-4-level off at those outputs: the correction is doing real work
    x = (rs.randn(30000) * 0.1).astype(np.float32)
    k, width = M.resampy_kernel_bank(44100, 16000)
    xp = np.pad(x, (width, width + 441 + 441))
    frames = np.lib.stride_tricks.sliding_window_view(xp, k.shape[1])[::441]
    plain = (frames @ k.T).reshape(-1)[:10884]
    want = R.librosa_resample(x, 44100, 16000)[:10884]
    bad = np.abs(plain - want) > 1e-5
    assert bad.any() and set(np.nonzero(bad)[0]) <= set(M.resampy_carries(10884, 44100, 16000).tolist())


def test_librosa_resample_restatement_behaves_like_a_resampler():
    """Defining properties of the restated kaiser_best resampler: a 1 kHz tone comes out as a 1 kHz tone (pass band flat to
    1e-2 away from the edges), a 9 kHz tone (above the new Nyquist) is rejected by > 60 dB, DC gain 1.003, and it stays within the
    transition-band difference of scipy's own Kaiser polyphase resampler on band-limited noise."""
    from scipy.signal import resample_poly

    from audiogpt_amd import mel as M
    sr = 44100
    t = np.arange(sr) / sr
    y = M.librosa_resample(np.sin(2 * np.pi * 1000 * t).astype(np.float32), sr, 16000)
    assert y.shape == (16000,)
    assert np.abs(y[1000:15000] - np.sin(2 * np.pi * 1000 * np.arange(16000) / 16000)[1000:15000]).max() < 1e-2
    y = M.librosa_resample(np.sin(2 * np.pi * 9000 * t).astype(np.float32), sr, 16000)
    assert np.abs(y[1000:15000]).max() < 1e-3
    y = M.librosa_resample(np.ones(sr, dtype=np.float32), sr, 16000)
    # (resampy steps its table by int(scale 512) = 185 where the exact stride is 185.76: the taps sit 0.4 % closer together than the
    # filter they sample and the gain is 1.003, not 1 -- a property of the algorithm as published, kept)
    assert 1.002 < y[1000:15000].min() and y[1000:15000].max() < 1.0035
    rs = np.random.RandomState(1)
    spec = np.fft.rfft(rs.randn(sr))
    spec[int(6000 * 1.0):] = 0                                   # noise band-limited to 6 kHz: inside both pass bands
    x = (np.fft.irfft(spec, sr) * 0.1).astype(np.float32)
    a = M.librosa_resample(x, sr, 16000)
    b = resample_poly(x, 160, 441).astype(np.float32)
    assert np.abs(a - b)[1000:15000].max() < 4e-3 * np.abs(b).max()         # 2.5e-3 measured, most of it the 1.003 gain
    assert np.abs(a / 1.0027 - b)[1000:15000].max() < 2e-3 * np.abs(b).max()


def test_bench_help_renders():
    """argparse expands `%` in help strings: a bare one made `python bench.py --help` raise ValueError (round 6)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--inflight" in r.stdout and "--cfg-split" in r.stdout, r.stderr[-800:]
