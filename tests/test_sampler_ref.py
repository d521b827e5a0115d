"""CPU self-test of tests/sampler_ref.py, the references tests/test_gpu_sampler_ops.py holds the step kernels to: the fp32
restatements stay within half of the GPU test's gate of the float64 ones on every input that test uses, the chained references
equal the committed oracle loops (oracle/ddim.py, oracle/diffsinger.py) bit for bit, the ring's slot arithmetic equals a deque, and
the inputs keep their distance from the thresholds the exact comparisons rely on.  No library, no device."""
from collections import deque

import numpy as np
import pytest
import torch

from tests import sampler_ref as R

F32, F64 = R.F32, R.F64
HALF = R.TOL / 2

# the chains' fp32-to-float64 distances as measured (the GPU module's docstring quotes them); the device gate is twice the
# distance of the very chain, computed at run time, and these bounds keep that gate from growing unnoticed
CHAIN_BOUND = {"ddim": 4e-7, "plms": 1.5e-6, "ddpm": 1.5e-6, "ds_plms": 2.5e-7, "ds_ddpm": 2e-7}


def pairs(ref):
    (a32, a64) = ref
    if isinstance(a32, tuple):
        return list(zip(a32, a64))
    return [(a32, a64)]


# ---------------------------------------------------------------------------------------------------- fp32 against float64

@pytest.mark.parametrize("shape,cfg", R.SHAPE_CFG)
def test_single_launches_fp32_within_half_the_gate(shape, cfg):
    for idx in R.IDX_ONE:
        for flag in (False, True):
            for a, b in pairs(R.prepare_case(shape, cfg, idx, flag)["ref"]) + pairs(R.ddim_case(shape, cfg, idx, flag)["ref"]):
                assert a.dtype == F32 and b.dtype == F64 and R.rel_max(a, b) <= HALF, (shape, cfg, idx, flag, R.rel_max(a, b))
    for slot in (-1, 0, 2):
        for a, b in pairs(R.ddim_case((2, 40, 0), False, 1, True, slot)["ref"]):
            assert R.rel_max(a, b) <= HALF


def test_update_entries_fp32_within_half_the_gate():
    for B, per in ((6, 40), (7, 42)):
        for clip in (False, True):
            for a, b in pairs(R.ddpm_update_case(B, per, clip)["ref"]):
                assert a.dtype == F32 and bool(torch.isfinite(a).all()) and R.rel_max(a, b) <= HALF, (B, per, clip, R.rel_max(a, b))
    for clip in (False, True):
        a, b = R.ds_update_case(6, 40, clip)["ref"]
        assert R.rel_max(a, b) <= HALF
    for B, per in ((4, 40), (3, 42)):
        k = R.encode_case(B, per)
        assert R.rel_max(*k["plain"]) <= HALF
        d = R.rel_max(*k["mom"])                # torch's fp32 exp against float64 (the expf exception of the GPU test)
        print("stochastic_encode from moments, fp32 to float64: %.3g" % d)
        assert d <= HALF


@pytest.mark.parametrize("case", R.CHAINS, ids=lambda c: "%s-%s-%s-%s" % (c[0], "x".join(map(str, c[1])), int(c[2]), c[3]))
def test_chain_distance_is_measured_and_bounded(case):
    k = R.chain_case(*case)
    d = R.chain_distance(k["c32"], k["c64"])
    print("%s: fp32 chain to float64 chain %.3g" % (case, d))
    assert 0 < d <= CHAIN_BOUND[case[0]], (case, d)
    assert [l["kind"] for l in k["c32"]] == [l["kind"] for l in k["c64"]]


def test_grid_stride_shapes_take_another_trip():
    (B4, per4), (B1, per1) = R.GRID_SHAPES
    assert per4 % 4 == 0 and B4 * per4 // 4 > 8192 * 256 and per1 % 4 != 0 and B1 * per1 > 8192 * 256
    assert R.EMB_W == 5 * 256 + 4          # five full trips of a 256-thread block and a partial sixth


# ---------------------------------------------------------------------------------------------------- against the oracle loops

class Counting:
    """apply_model / denoise_fn for the oracle loops: the k-th call returns the synthetic model's k-th evaluation."""

    def __init__(self, model):
        self.model, self.k = model, 0

    def __call__(self, x, t, c=None, **kw):
        out = self.model(self.k, x.reshape(x.shape[0], -1), F32).reshape(x.shape)
        self.k += 1
        return out


@pytest.mark.parametrize("eta", (0.0, R.ETA))
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("cfg", (False, True))
def test_ddim_chain_equals_the_oracle_loop(eta, masked, cfg):
    """oracle.ddim.ddim_sample (S = 6: the seven indices the reference's uniform discretisation gives) driven by the same callable:
    every step's latent and the logged intermediates, bit for bit."""
    from oracle import ddim as OD
    B, per = 2, 40
    ac = OD.alphas_cumprod()
    steps = OD.ddim_timesteps(6, ac.shape[0])
    S = len(steps)
    nB = 2 * B if cfg else B
    sch = R.ddim_schedule(S, eta, steps)
    assert bool((1.0 - sch["ap"].double() - sch["sig"].double() ** 2 > 0).all())
    d = R.latent_inputs(B, per, 0, cfg, S, 5)
    model = R.SyntheticModel(nB, per, S, 6)
    slots, n_log = R.ddim_log_slots(S, 3)
    kw = {}
    if masked:
        kw.update(mask=d["mask"], x0=d["x0"], noise_q=d["noise_q"])
    if eta > 0:
        kw.update(noise_p=d["noise_p"], temperature=R.TEMPERATURE)
    with R.torch_sqrt():          # (the oracle's own primitive: sampler_ref.sqrt says why the references do not use it otherwise)
        chain = R.ddim_chain(model, sch, d["x"], nB, R.SCALE, F32, slots=slots, **kw)
    img = lambda t: None if t is None else t.reshape(*t.shape[:-1], 1, 1, per)
    trace = []
    okw = dict(mask=img(d["mask"]), x0=img(d["x0"]), noise_q=img(d["noise_q"])) if masked else {}
    if eta > 0:
        okw.update(noise_p=img(d["noise_p"]), temperature=R.TEMPERATURE)
    x, inter = OD.ddim_sample(Counting(model), ac, 6, img(d["x"]), torch.zeros(B, 1), torch.zeros(B, 1) if cfg else None, R.SCALE, eta,
                              trace=trace, log_every_t=3, **okw)
    mine = [l for l in chain if l["kind"] == "ddim"]
    assert len(mine) == len(trace) == S
    for l, t in zip(mine, trace):
        assert torch.equal(l["expect"]["x"], t.reshape(B, per)), l["idx"]
    logged = [l for l in mine if "log_x" in l["expect"]]
    assert [l["expect"]["log_x"][0] for l in logged] == list(range(n_log)) and len(inter["x_inter"]) == n_log + 1
    for l, lx, l0 in zip(logged, inter["x_inter"][1:], inter["pred_x0"][1:]):
        assert torch.equal(l["expect"]["log_x"][1], lx.reshape(B, per)) and torch.equal(l["expect"]["log_x0"][1], l0.reshape(B, per))


def test_ds_plms_chain_equals_the_oracle_loop():
    """oracle.diffsinger.plms_sample with K_step = 60, interval = 10 (t = 50 .. 0) driven by the same callable, bit for bit."""
    from oracle import diffsinger as ODS
    B, per = 2, 40
    ac = ODS.alphas_cumprod(R.DS_TIMESTEPS, 0.06)
    x_T = R.randn(R.gen(7), B, per)
    model = R.SyntheticModel(B, per, 8, 8)
    with R.torch_sqrt():
        chain = R.ds_plms_chain(model, ac, x_T, 50, 10, F32)
    trace = []
    ODS.plms_sample(Counting(model), ac, x_T.reshape(B, 1, 4, 10), None, 60, 10, trace=trace)
    mine = [l for l in chain if l["kind"] == "ds_plms" and l["mode"] != 1]
    assert len(mine) == len(trace) == 6
    for l, t in zip(mine, trace):
        assert torch.equal(l["expect"]["x"], t.reshape(B, per))
    assert chain[-1]["expect"]["st"] == [-10, 6, 0] and chain[-1]["expect"]["t_slot"] == 0.0


def test_plms_e_prime_equals_the_oracle_line():
    """The Adams-Bashforth lines of plms.py:226-232 in fp32, against torch's evaluation of the reference's own expressions."""
    g = R.gen(9)
    e, h1, h2, h3 = (R.randn(g, 64) for _ in range(4))
    assert torch.equal(R.plms_e_prime(e, [h1], F32), (3 * e - h1) / 2)
    assert torch.equal(R.plms_e_prime(e, [h2, h1], F32), (23 * e - 16 * h1 + 5 * h2) / 12)
    assert torch.equal(R.plms_e_prime(e, [h3, h2, h1], F32), (55 * e - 59 * h1 + 37 * h2 - 9 * h3) / 24)
    assert torch.equal(R.plms_e_prime(e, ("next", h1), F32), (e + h1) / 2)


# ---------------------------------------------------------------------------------------------------- the ring

def test_ring_slots_against_a_deque():
    """i % 3, (i + 2) % 3, (i + 1) % 3 for i = 0 .. 8: the ring holds what deque(maxlen=3) holds, h_k = the e_t of step i - k, and
    h3 shares the slot this step's e_t is written to."""
    ring, old = [None] * 3, deque(maxlen=3)
    for i in range(9):
        w, h1, h2, h3 = R.ring_slots(i)
        assert len({h1, h2, h3}) == 3 and w == h3
        for k, slot in enumerate((h1, h2, h3), start=1):
            if len(old) >= k:
                assert ring[slot] == old[-k] == i - k, (i, k)
        ring[w] = i
        old.append(i)
    assert sorted(ring) == [6, 7, 8]


# ---------------------------------------------------------------------------------------------------- thresholds

def test_inputs_keep_their_distance_from_the_thresholds():
    """The clamp cases place exact +-1.0 on purpose (and +-2) and otherwise the first launch's x_recon stays 1e-3 away from +-1;
    masks hold exact 0 and 1 and fractions; every 1 - a_prev - sigma^2 in use is positive; every draw is visibly its own."""
    for S, eta in ((R.S_ONE, R.ETA), (R.S_ONE, 0.0), (R.PLMS_S, 0.0), (5, 0.0)):
        sch = R.ddim_schedule(S, eta)
        assert bool((1.0 - sch["ap"].double() - sch["sig"].double() ** 2 > 0).all()) and bool((sch["a"] > 0).all())
        assert (eta == 0) == bool((sch["sig"] == 0).all())
    for B, per in ((6, 40), (7, 42)):
        k = R.ddpm_update_case(B, per, True)
        rows = R.ddpm_rows(k["tabs"], R.TEMPERATURE)
        raw = torch.stack([rows[int(k["t"][b]), 0] * k["x"][b] - rows[int(k["t"][b]), 1] * k["e"][b] for b in range(B)])
        assert bool((raw[:, 0] == 1.0).all() and (raw[:, 1] == -1.0).all() and (raw[:, 2] == 2.0).all() and (raw[:, 3] == -2.0).all())
        assert bool(((raw[:, 4:].abs() - 1.0).abs() > 1e-3).all())
        assert bool(torch.isnan(k["z"][k["t"] == 0]).all()) and int((k["t"] == 0).sum()) >= 1
    for v in (1, 3):
        k = R.chain_case("ddpm", (2, 40, 0), True, v)
        first = k["c64"][1]["expect"]["log_x0"][1]
        tab = k["tab"]
        e0 = R.cfg_eps(*k["model"](0, torch.cat([k["x_T"]] * 2), F32).chunk(2), R.SCALE, F32)
        raw = tab[R.DDPM_START, 0] * k["x_T"] - tab[R.DDPM_START, 1] * e0
        assert bool((raw[:, 0] == 1.0).all() and (raw[:, 1] == -1.0).all() and (raw[:, 2:4].abs() == 2.0).all())
        assert bool(((raw[:, 4:].abs() - 1.0).abs() > 1e-3).all()) and bool((first.abs() <= 1.0).all())
        assert bool((raw[:, 4:].abs() > 1.0).any()) and bool((raw[:, 4:].abs() < 1.0).any())
    d = R.latent_inputs(2, 40, 0, True, 4, 11)
    m = d["mask"]
    assert bool((m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any())
    means = d["noise_p"].mean(dim=(1, 2))
    assert bool((means[1:] - means[:-1] > R.DRAW_OFFSET / 2).all())
    k = R.encode_case(4, 40)
    assert k["moments"][0, 1, :4].tolist() == [-31.0, -30.0, 20.0, 21.0]


def test_table_layouts():
    """The three rows as the kernels read them: 8 floats by DDIM index, 9 by DDPM timestep, 5 for DiffSinger."""
    sch = R.ddim_schedule(4, R.ETA)
    slots, n = R.ddim_log_slots(4, 2)
    assert slots == [2, -1, 1, 0] and n == 3
    rows = R.ddim_coef_rows(sch, slots)
    assert rows.shape == (4, 8) and rows[:, 7].tolist() == [0, 1, 2, 3] and rows[:, 6].tolist() == [2, -1, 1, 0]
    assert torch.equal(rows[:, 3], R.sqrt(1 - sch["a"])) and R.rel_max(rows[:, 3], sch["soma"]) < 2e-7 and torch.equal(rows[:, 4], sch["sq_ac"]) and torch.equal(rows[:, 2], sch["sig"])
    assert bool((R.ddim_coef_rows(sch, masked=False)[:, 4:6] == 0).all())
    tabs = R.posterior_tables(6)
    t9 = R.ddpm_rows(tabs, 0.7, [0, -1, 1, -1, 2, 3])
    assert t9.shape == (6, 9) and float(t9[0, 4]) == 0.0 and bool((t9[1:, 4] > 0).all()) and bool((t9[:, 5] == np.float32(0.7)).all())
    assert R.rel_max(t9[1:, 4], torch.exp(0.5 * tabs["posterior_log_variance_clipped"][1:].double())) < 1e-6
    assert torch.equal(t9[:, 6], tabs["sqrt_alphas_cumprod"]) and t9[:, 8].tolist() == [0, -1, 1, -1, 2, 3]
    assert R.ds_rows(tabs).shape == (6, 5) and torch.equal(R.ds_rows(tabs), t9[:, :5])
