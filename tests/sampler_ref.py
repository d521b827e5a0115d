"""References of the sampling loops' step kernels (csrc/sampler_steps.hip; tests/test_gpu_sampler_ops.py through maa_op_sampler_step, maa_ddim_update,
maa_ddim_stochastic_encode, maa_ddpm_update, maa_ds_ddpm_update), written from the reference's own lines and not from the kernels:

  ldm/models/diffusion/ddim.py        p_sample_ddim (:199, :210-225), the mask blend of ddim_sampling (:147-150), stochastic_encode
  ldm/models/diffusion/plms.py        p_sample_plms (:218-236), get_x_prev_and_pred_x0 (:199-216)
  ldm/models/diffusion/ddpm_audio.py  p_sample (:749-777), p_mean_variance's clamp (:737), q_posterior, the blend of the loop (:873-875)
  modules/diff/shallow_diffusion_tts.py   p_sample_plms / get_x_pred (:169-204), p_sample (:160-166)

Every operation exists twice through one body and a dtype: `dt = F32` evaluates one correctly rounded fp32 operation at a time in
the reference's term order (every scalar is a 0-dim fp32 tensor: no Python float enters an expression, `one(dt)` and `num(k, dt)`
stand for the literals), `dt = F64` the same formula in float64, fed from the fp32 inputs and fp32 table values.  The `*_f32` /
`*_f64` names are those two.  The fp32 form is a bit-for-bit oracle of the kernels (elementwise IEEE arithmetic, no contraction);
the float64 form is the independent second one.

The chained references (`*_chain`) return the launches of a trajectory in order, each with the buffers it must leave behind, so a
driver can run the same launches and compare after every one.  The "model" between launches is synthetic:
eps_k = a_k * x + b_k * randn_k (SyntheticModel), only the step kernels are under test."""
import ctypes
import ctypes.util
import functools
from collections import deque

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64

TOL = 1e-5                  # the project's elementwise operator gate, rel-max against float64, for one launch
SCALE = 3.0                 # classifier-free guidance
TEMPERATURE = 0.7
ETA = 0.5
# (B, per, per_c): one vector; V = 4; per % 4 != 0 (a sample boundary inside a would-be vector); concat, V = 4; per_in % 4 != 0
SHAPES = [(1, 4, 0), (2, 40, 0), (3, 42, 0), (2, 40, 20), (2, 40, 6)]
GRID_SHAPES = [(2, 4194312), (1, 2097153)]      # V = 4 with more than 8192 * 256 vectors; V = 1 with more than 8192 * 256 elements
EMB_W = 1284                # 5 * 256 + 4: five full trips of a 256-thread block and a partial sixth
DRAW_OFFSET = 4.0           # draw k of a noise buffer is randn + DRAW_OFFSET * (k + 1): a wrong draw is visible


def one(dt):
    return torch.ones((), dtype=dt)


def num(k, dt):
    """The literal k of a reference line (3, 23, 16, ... , 2, 12, 24: exact in fp32)."""
    assert float(np.float32(k)) == float(k)
    return torch.tensor(float(k), dtype=F32).to(dt)


def up(t, dt):
    """An fp32 input or table value, widened to the working dtype (exact)."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    assert t.dtype in (F32, dt), t.dtype          # (a chain's own state is already in the working dtype)
    return t.to(dt)


_SQRT = [None]


def sqrt(t):
    """The correctly rounded square root: formed in float64 by numpy and rounded once (exact for fp32 operands: 53 >= 2 * 24 + 2).
    torch's own fp32 sqrt on the CPU is NOT used: on some hosts its vector kernel is an ulp off on about one value in six
    (measured on the device's host: 704 of 4096 values of |randn| + 0.1), while its add, sub, mul and div are IEEE everywhere
    they were measured.  The kernels' sqrtf is correctly rounded, so the oracle has to be."""
    if _SQRT[0] is not None:
        return _SQRT[0](t)
    return torch.as_tensor(np.sqrt(np.asarray(t.numpy(), dtype=np.float64))).to(t.dtype)


class torch_sqrt:
    """`with torch_sqrt():` the references take torch.sqrt, the primitive the committed oracle loops use -- for the cross-checks
    against those loops, which tie term order and formulas and run on one host with one sqrt."""

    def __enter__(self):
        _SQRT[0] = torch.sqrt

    def __exit__(self, *exc):
        _SQRT[0] = None


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F32)


# ------------------------------------------------------------------------------------------------ schedules and table layouts

def ddim_schedule(S, eta=0.0, steps=None):
    """fp32 tables by DDIM index of an S-step schedule over the 1000-step linear one (oracle.ddim: util.py:46-74, ddim.py:46-52).
    steps None: exactly S indices, k * (1000 // S) + 1."""
    from oracle import ddim as OD
    ac = OD.alphas_cumprod()
    if steps is None:
        steps = np.arange(S) * (1000 // S) + 1
    a, ap, sig, soma = OD.ddim_tables(ac, steps, eta)
    sq_ac, sq_1mac = OD.q_sample_tables(ac, steps)
    return dict(steps=np.asarray(steps), a=a, ap=ap, sig=sig, soma=soma, sq_ac=sq_ac, sq_1mac=sq_1mac)


def ddim_log_slots(S, log_every_t):
    """ddim.py:161: index % log_every_t == 0 or index == S - 1, numbered in visiting order (index S - 1 first); -1: not logged."""
    slots, n = [-1] * S, 0
    for i in range(S - 1, -1, -1):
        if log_every_t and (i % log_every_t == 0 or i == S - 1):
            slots[i] = n
            n += 1
    return slots, n


def ddim_coef_rows(sch, slots=None, masked=True):
    """The loop's coefficient table, one row per DDIM index (csrc/ddim.cpp, Loop):
    [S, 8] = {a_t, a_prev, sigma, sqrt(1 - a_t) in fp32, sqrt_ac, sqrt_1mac (0 without a mask), log slot (-1: none), index}."""
    S = sch["a"].shape[0]
    rows = torch.zeros(S, 8, dtype=F32)
    rows[:, 0], rows[:, 1], rows[:, 2] = sch["a"], sch["ap"], sch["sig"]
    rows[:, 3] = sqrt(one(F32) - sch["a"])
    if masked:
        rows[:, 4], rows[:, 5] = sch["sq_ac"], sch["sq_1mac"]
    rows[:, 6] = torch.tensor([-1.0] * S if slots is None else [float(s) for s in slots])
    rows[:, 7] = torch.arange(S, dtype=F32)
    return rows


def identity_coef_rows(T):
    """What the ancestral loop hands the prepare kernel: the identity schedule, only the index matters."""
    return ddim_coef_rows(dict(a=torch.ones(T), ap=torch.ones(T), sig=torch.zeros(T)), masked=False)


def posterior_tables(T, beta_lo=0.05, beta_hi=0.4):
    """ddpm.py:115-155 on a T-step linear schedule: fp64 arithmetic, fp32 buffers, under the reference's names."""
    betas = np.linspace(beta_lo, beta_hi, T)
    alphas = 1.0 - betas
    ac = np.cumprod(alphas)
    ac_prev = np.append(1.0, ac[:-1])
    var = betas * (1.0 - ac_prev) / (1.0 - ac)
    f = lambda v: torch.tensor(v, dtype=F32)
    return dict(sqrt_recip_alphas_cumprod=f(np.sqrt(1.0 / ac)), sqrt_recipm1_alphas_cumprod=f(np.sqrt(1.0 / ac - 1)),
                posterior_mean_coef1=f(betas * np.sqrt(ac_prev) / (1.0 - ac)),
                posterior_mean_coef2=f((1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac)),
                posterior_log_variance_clipped=f(np.log(np.maximum(var, 1e-20))),
                sqrt_alphas_cumprod=f(np.sqrt(ac)), sqrt_one_minus_alphas_cumprod=f(np.sqrt(1.0 - ac)))


def host_expf(v):
    """exp of fp32 values as the library's host code forms it (std::exp(float) = the C library's expf)."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    return torch.tensor([libm.expf(float(x)) for x in v], dtype=F32)


def posterior_sd(tabs):
    """nonzero_mask * (0.5 * posterior_log_variance_clipped).exp() per timestep (0 at t = 0), fp32."""
    sd = host_expf(num(0.5, F32) * tabs["posterior_log_variance_clipped"])
    sd[0] = 0.0
    return sd


def ddpm_rows(tabs, temperature=1.0, slots=None, masked=True):
    """The ancestral loop's table (DDPM_TAB_W = 9), one row per timestep:
    [T, 9] = {sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sd (0 at t = 0), temperature, sqrt_ac, sqrt_1mac, log slot (-1: none)}."""
    T = tabs["posterior_mean_coef1"].shape[0]
    rows = torch.zeros(T, 9, dtype=F32)
    for k, name in enumerate(("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2")):
        rows[:, k] = tabs[name]
    rows[:, 4] = posterior_sd(tabs)
    rows[:, 5] = torch.tensor(temperature, dtype=F32).expand(T)
    if masked:
        rows[:, 6], rows[:, 7] = tabs["sqrt_alphas_cumprod"], tabs["sqrt_one_minus_alphas_cumprod"]
    rows[:, 8] = torch.tensor([-1.0] * T if slots is None else [float(s) for s in slots])
    return rows


def ds_rows(tabs):
    """DiffSinger's ancestral table: [T, 5] = {sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, sigma (0 in row 0)}."""
    return ddpm_rows(tabs)[:, :5].contiguous()


# ------------------------------------------------------------------------------------------------ one launch each

def cfg_eps(eu, ec, scale, dt):
    """ddim.py:199: e_t = e_t_uncond + unconditional_guidance_scale * (e_t - e_t_uncond); ec None: no guidance."""
    eu = up(eu, dt)
    if ec is None:
        return eu
    return eu + up(torch.tensor(scale, dtype=F32), dt) * (up(ec, dt) - eu)


def mask_blend(x, mask, x0, z, sq_ac, sq_1mac, dt):
    """ddim.py:149-150 / ddpm_audio.py:874-875: img_orig = q_sample(x0, ts) = sqrt_ac x0 + sqrt_1mac z (ddpm.py:272-275);
    img = img_orig * mask + (1. - mask) * img."""
    img_orig = up(sq_ac, dt) * up(x0, dt) + up(sq_1mac, dt) * up(z, dt)
    m = up(mask, dt)
    return img_orig * m + (one(dt) - m) * up(x, dt)


def prepare(x, concat, nB, row, dt, mask=None, x0=None, z=None):
    """The step's model input [nB, per + per_c]: the (blended) latent, then the concat channels; nB = 2 B repeats the rows
    (ddim.py:177: torch.cat([x] * 2))."""
    B = x.shape[0]
    row = up(row, dt)
    v = up(x, dt)
    if mask is not None:
        v = mask_blend(v, mask, x0, z, row[4], row[5], dt)
    if concat is not None and concat.shape[1] > 0:
        v = torch.cat([v, up(concat, dt)], dim=1)
    return torch.cat([v] * (nB // B), dim=0)


def x_prev_and_pred_x0(x, e, row, dt, z=None, temperature=None):
    """ddim.py:216-225 / plms.py:207-216: pred_x0 = (x - sqrt_one_minus_at * e_t) / a_t.sqrt(); dir_xt = (1. - a_prev -
    sigma_t**2).sqrt() * e_t; noise = sigma_t * z * temperature; x_prev = a_prev.sqrt() * pred_x0 + dir_xt + noise.
    z None: the noise term is not formed (sigma = 0 in the reference adds a zero)."""
    row, x, e = up(row, dt), up(x, dt), up(e, dt)
    a_t, a_prev, sigma_t, somat = row[0], row[1], row[2], row[3]
    pred_x0 = (x - somat * e) / sqrt(a_t)
    dir_xt = sqrt(one(dt) - a_prev - sigma_t * sigma_t) * e
    x_prev = sqrt(a_prev) * pred_x0 + dir_xt
    if z is not None:
        x_prev = x_prev + sigma_t * up(z, dt) * up(torch.tensor(temperature, dtype=F32), dt)
    return x_prev, pred_x0


def ddim_step(x, eu, ec, scale, row, dt, z=None, temperature=None):
    """p_sample_ddim after the model: (x_prev, pred_x0).  x: the latent rows of the step's model input."""
    return x_prev_and_pred_x0(x, cfg_eps(eu, ec, scale, dt), row, dt, z, temperature)


def plms_e_prime(e, old, dt):
    """plms.py:223-232 with old = old_eps (newest last) and, for len(old) == 0, e_next given as old = ('next', e_next)."""
    e = up(e, dt)
    old = (old[0], up(old[1], dt)) if isinstance(old, tuple) else [up(o, dt) for o in old]
    if isinstance(old, tuple):
        return (e + old[1]) / num(2, dt)
    if len(old) == 1:
        return (num(3, dt) * e - old[-1]) / num(2, dt)
    if len(old) == 2:
        return (num(23, dt) * e - num(16, dt) * old[-1] + num(5, dt) * old[-2]) / num(12, dt)
    return (num(55, dt) * e - num(59, dt) * old[-1] + num(37, dt) * old[-2] - num(9, dt) * old[-3]) / num(24, dt)


def ring_slots(i):
    """Slots of the three-slab ring at step i: (where e_t of step i goes, h1, h2, h3) = (i % 3, (i + 2) % 3, (i + 1) % 3, i % 3)."""
    return i % 3, (i + 2) % 3, (i + 1) % 3, i % 3


def ddpm_step(x, e, z, row, clip, dt):
    """ddpm_audio.py p_sample: x_recon = sqrt_recip_ac x - sqrt_recipm1_ac e (clamped when clip); model_mean = coef1 x_recon + coef2 x;
    x' = model_mean + (nonzero_mask * exp(0.5 logvar)) * (z * temperature).  row = {.., sd, temperature}: sd = 0 is the t = 0 row,
    where the reference multiplies its draw by zero and the kernels' contract is not to read it.  Returns (x', x_recon)."""
    row, x, e = up(row, dt), up(x, dt), up(e, dt)
    x_recon = row[0] * x - row[1] * e
    if clip:
        x_recon = x_recon.clamp(-1.0, 1.0)
    mean = row[2] * x_recon + row[3] * x
    if float(row[4]) != 0.0:
        mean = mean + row[4] * (up(z, dt) * row[5])
    return mean, x_recon


def ds_ddpm_step(x, e, z, row, clip, dt):
    """shallow_diffusion_tts.py:134-166: as ddpm_step without temperature, `mean + nonzero_mask * (0.5 * logvar).exp() * noise`
    (the product with the draw is formed at t = 0 too)."""
    row, x, e = up(row, dt), up(x, dt), up(e, dt)
    x_recon = row[0] * x - row[1] * e
    if clip:
        x_recon = x_recon.clamp(-1.0, 1.0)
    return row[2] * x_recon + row[3] * x + row[4] * up(z, dt)


def ds_x_pred(ac, x, noise_t, t, interval, dt):
    """get_x_pred (:174-185), the reference's expression term for term:
    x_delta = (a_prev - a_t) * ((1 / (a_t_sq * (a_t_sq + a_prev_sq))) * x - 1 / (a_t_sq * (((1 - a_prev) * a_t).sqrt() +
    ((1 - a_t) * a_prev).sqrt())) * noise_t)."""
    x, noise_t = up(x, dt), up(noise_t, dt)
    a_t = up(ac[t], dt)
    a_prev = one(dt) if t < interval else up(ac[max(t - interval, 0)], dt)
    a_t_sq, a_prev_sq = sqrt(a_t), sqrt(a_prev)
    x_delta = (a_prev - a_t) * ((one(dt) / (a_t_sq * (a_t_sq + a_prev_sq))) * x -
                                one(dt) / (a_t_sq * (sqrt((one(dt) - a_prev) * a_t) + sqrt((one(dt) - a_t) * a_prev))) * noise_t)
    return x + x_delta


def ds_e_prime(e, hist, dt):
    """:193-199 with hist = noise_list (newest last); a tuple ('prev', e_prev) is the first step's corrector."""
    return plms_e_prime(e, hist, dt)


def stochastic_encode(x0, t, sqrt_a, sqrt_1ma, noise, dt, moments=None, scale_factor=None, n_post=None):
    """ddim.py:240-241 with one index per sample; moments [B, 2, per]: x0 = scale_factor * (mean + exp(0.5 * clamp(logvar, -30, 20))
    * n_post) (DiagonalGaussianDistribution.sample, get_first_stage_encoding).  Returns (out, x0)."""
    if moments is not None:
        mean, logvar = up(moments[:, 0], dt), up(moments[:, 1], dt)
        std = torch.exp(num(0.5, dt) * torch.clamp(logvar, -30.0, 20.0))
        x0 = up(torch.tensor(scale_factor, dtype=F32), dt) * (mean + std * up(n_post, dt))
    else:
        x0 = up(x0, dt)
    ca, cb = up(sqrt_a, dt)[t].reshape(-1, 1), up(sqrt_1ma, dt)[t].reshape(-1, 1)
    return ca * x0 + cb * up(noise, dt), x0


for _name in ("prepare", "ddim_step", "ddpm_step", "ds_ddpm_step", "ds_x_pred", "stochastic_encode", "x_prev_and_pred_x0"):
    globals()[_name + "_f32"] = functools.partial(globals()[_name], dt=F32)
    globals()[_name + "_f64"] = functools.partial(globals()[_name], dt=F64)


# ------------------------------------------------------------------------------------------------ inputs

def latent_inputs(B, per, per_c, cfg, n_draws, seed, big=False):
    """Deterministic inputs of one launch on a [B, per] latent: x, concat, eps halves, mask (exact 0 and 1 and fractions), x0, and
    n_draws draws of the two noises, draw k offset by DRAW_OFFSET * (k + 1)."""
    g = gen(seed)
    d = dict(x=randn(g, B, per), concat=randn(g, B, per_c), eu=randn(g, B, per), ec=randn(g, B, per) if cfg else None)
    if big:
        return d
    m = torch.rand(B, per, generator=g, dtype=F32)
    m[:, 0::3] = 0.0
    m[:, 1::3] = 1.0
    d["mask"], d["x0"] = m, randn(g, B, per)
    off = (torch.arange(n_draws, dtype=F32) + 1).reshape(-1, 1, 1) * DRAW_OFFSET
    d["noise_q"], d["noise_p"] = randn(g, n_draws, B, per) + off, randn(g, n_draws, B, per) + off
    return d


class SyntheticModel:
    """eps_k = a_k * x + b_k * randn_k for the k-th evaluation on `rows` rows of `per` floats: a_k one factor per row (the two
    guidance halves differ), every evaluation an independent draw.  `terms(k)` gives (a_k [rows, 1], b_k, randn_k) as fp32;
    evaluating is the caller's: a_k * x + b_k * r in its own dtype and on its own device."""

    def __init__(self, rows, per, n_evals, seed):
        g = gen(seed)
        self.a = torch.rand(n_evals, rows, 1, generator=g, dtype=F32) * 0.5 + 0.25
        self.b = torch.rand(n_evals, generator=g, dtype=F32) * 0.5 + 0.5
        self.r = randn(g, n_evals, rows, per)

    def terms(self, k):
        return self.a[k], self.b[k], self.r[k]

    def __call__(self, k, x, dt):
        a, b, r = self.terms(k)
        return up(a, dt) * x + up(b, dt) * up(r, dt)


def unit_clamp_x(c0):
    """An fp32 x with fl(c0 * x) == 1.0 exactly, searched within a few ulps of 1 / c0 (not every c0 has one: the tables in use do,
    and test_sampler_ref.py asserts the planted products)."""
    c0 = np.float32(c0)
    x = np.float32(1.0) / c0
    cands = [x]
    lo = hi = x
    for _ in range(8):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(4))
        cands += [lo, hi]
    for c in cands:
        if np.float32(c0 * c) == np.float32(1.0):
            return float(c)
    raise AssertionError("no fp32 x with c0 * x == 1 near 1 / %r" % c0)


def plant_clamp(x, e, c0):
    """Elements 0..3 of every sample: x_recon = c0 x - c1 * 0 lands on +1, -1 exactly, and on +-2 (beyond)."""
    u = unit_clamp_x(c0)
    x, e = x.clone(), e.clone()
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = u, -u, 2 * u, -2 * u
    e[:, :4] = 0.0
    return x, e


# ------------------------------------------------------------------------------------------------ chained trajectories

def ddim_chain(model, sch, x_T, nB, scale, dt, concat=None, mask=None, x0=None, noise_q=None, noise_p=None, temperature=None,
               slots=None, plms=False):
    """The DDIM (plms: PLMSSampler) trajectory over all S indices as launches in order.  Each launch is a dict: kind, idx, `eval`
    (the model evaluation that precedes it, None: none) and `expect`, the buffers it leaves: xin [nB, per_in], coef [8], cur_t,
    x [B, per], step, and for logged steps log_x / log_x0 (slab, tensor); PLMS adds ring [3, B, per], x_save (= x), e_keep."""
    S = sch["a"].shape[0]
    B, per = x_T.shape
    rows = ddim_coef_rows(sch, slots, masked=mask is not None)
    cfg = nB == 2 * B
    x = up(x_T, dt)
    out = []
    ring = [None, None, None]
    old = deque(maxlen=3)
    k = 0

    def guided(eps):
        return cfg_eps(eps[:B], eps[B:] if cfg else None, scale, dt)

    for i in range(S):
        idx = S - 1 - i
        row = rows[idx]
        z_q = noise_q[i] if mask is not None else None
        xin = prepare(x, concat, nB, row, dt, mask, x0, z_q)
        out.append(dict(kind="ddim_prepare", idx=idx, eval=None,
                        expect=dict(xin=xin, coef=row, cur_t=float(sch["steps"][idx]))))
        xb = xin[:B, :per]
        e = guided(model(k, xin[:, :per], dt))
        ev, k = k, k + 1
        slot = int(row[6])
        if not plms:
            z_p = noise_p[i] if noise_p is not None else None
            x, pred = x_prev_and_pred_x0(xb, e, row, dt, z_p, temperature)
            exp = dict(x=x, step=idx - 1)
        elif i == 0:
            x_mid, _ = x_prev_and_pred_x0(xb, e, row, dt)
            xin_mid = xin.clone()
            xin_mid[:, :per] = torch.cat([x_mid] * (nB // B), dim=0)
            ring[0] = e
            out.append(dict(kind="plms_euler_mid", idx=idx, eval=ev,
                            expect=dict(xin=xin_mid, x=xb, ring=list(ring), cur_t=float(sch["steps"][max(idx - 1, 0)]))))
            e_next = guided(model(k, xin_mid[:, :per], dt))
            ev, k = k, k + 1
            x, pred = x_prev_and_pred_x0(xb, plms_e_prime(e, ("next", e_next), dt), row, dt)
            exp = dict(x=x, step=idx - 1, ring=list(ring))
            old.append(e)
        else:
            w, h1, h2, h3 = ring_slots(i)
            assert all(ring[s] is o for s, o in zip((h1, h2, h3), reversed(old)))      # the ring holds what old_eps holds
            x, pred = x_prev_and_pred_x0(xb, plms_e_prime(e, list(old), dt), row, dt)
            ring[w] = e
            old.append(e)
            exp = dict(x=x, step=idx - 1, ring=list(ring))
        if slot >= 0:
            exp["log_x"], exp["log_x0"] = (slot, x), (slot, pred)
        kind = "ddim" if not plms else ("plms_euler_final" if i == 0 else "plms")
        out.append(dict(kind=kind, idx=idx, eval=ev, expect=exp))
    return out


def ddpm_chain(model, tab, x_T, start, clip, dt, nB=None, scale=1.0, mask=None, x0=None, noise_q=None, noise_p=None):
    """The ancestral trajectory t = start .. 0 as launches (prepare without a blend, then the step with the blend after it).
    tab: ddpm_rows [T, 9].  A logged step (tab[t, 8] >= 0) logs x' after the blend and x_recon after the clamp."""
    B, per = x_T.shape
    nB = B if nB is None else nB
    cfg = nB == 2 * B
    ident = identity_coef_rows(tab.shape[0])
    x = up(x_T, dt)
    out = []
    for v, t in enumerate(range(start, -1, -1)):
        xin = prepare(x, None, nB, ident[t], dt)
        out.append(dict(kind="ddim_prepare", idx=t, eval=None, expect=dict(xin=xin, coef=ident[t], cur_t=float(t))))
        eps = model(v, xin, dt)
        e = cfg_eps(eps[:B], eps[B:] if cfg else None, scale, dt)
        xp, xr = ddpm_step(xin[:B], e, noise_p[v], tab[t], clip, dt)
        if mask is not None:
            row = up(tab[t], dt)
            xp = mask_blend(xp, mask, x0, noise_q[v], row[6], row[7], dt)
        x = xp
        exp = dict(x=x, step=t - 1)
        if int(tab[t, 8]) >= 0:
            exp["log_x"], exp["log_x0"] = (int(tab[t, 8]), x), (int(tab[t, 8]), xr)
        out.append(dict(kind="ddpm", idx=t, eval=v, expect=exp))
    return out


def ds_plms_chain(model, ac, x_T, t0, interval, dt):
    """DiffSinger's PLMS trajectory t = t0, t0 - interval, ... >= 0 as launches: predictor (mode 1), corrector (mode 2), advance,
    then multistep (mode 0) + advance.  expect: x, x_out, hist [3] by ring slot (None: never written), st = [t, count, head],
    t_slot."""
    x = up(x_T, dt)
    out = []
    hist = [None, None, None]
    noise_list = []
    st = [t0, 0, 0]
    k = 0
    t = t0
    while t >= 0:
        e = model(k, x, dt)
        ev, k = k, k + 1
        if not noise_list:
            x_pred = ds_x_pred(ac, x, e, t, interval, dt)
            out.append(dict(kind="ds_plms", mode=1, eval=ev, on="x", expect=dict(x=x, x_out=x_pred, hist=list(hist), st=list(st))))
            e_prev = model(k, x_pred, dt)
            ev, k = k, k + 1
            e_prime = ds_e_prime(e, ("prev", e_prev), dt)
            mode = 2
        else:
            e_prime = ds_e_prime(e, noise_list, dt)
            mode = 0
        x = ds_x_pred(ac, x, e_prime, t, interval, dt)
        noise_list.append(e)
        hist[(st[2] + 1) % 3] = e
        out.append(dict(kind="ds_plms", mode=mode, eval=ev, on="x_out" if mode == 2 else "x",
                        expect=dict(x=x, hist=list(hist), st=list(st))))
        t -= interval
        st = [t, st[1] + 1, (st[2] + 1) % 3]
        out.append(dict(kind="ds_advance", eval=None, expect=dict(x=x, hist=list(hist), st=list(st), t_slot=float(max(t, 0)))))
    return out


def ds_ddpm_chain(model, tab, x_T, start, clip, noise, dt):
    """DiffSinger's ancestral trajectory t = start .. 0: the step with draw start - t, then advance with interval 1."""
    x = up(x_T, dt)
    out = []
    for k, t in enumerate(range(start, -1, -1)):
        x = ds_ddpm_step(x, model(k, x, dt), noise[k], tab[t], clip, dt)
        out.append(dict(kind="ds_ddpm", eval=k, expect=dict(x=x, st=[t, k, k % 3])))
        out.append(dict(kind="ds_advance", eval=None, expect=dict(x=x, st=[t - 1, k + 1, (k + 1) % 3], t_slot=float(max(t - 1, 0)))))
    return out


def rel_max(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.to(F64), b.to(F64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def chain_distance(c32, c64):
    """The largest rel-max distance between the tensor buffers two chains (fp32 / fp64, same launches) leave behind."""
    worst = 0.0
    for a, b in zip(c32, c64):
        assert a["kind"] == b["kind"]
        for key, v in a["expect"].items():
            w = b["expect"][key]
            if isinstance(v, tuple):
                v, w = v[1], w[1]
            for p, q in zip(v, w) if isinstance(v, list) else [(v, w)]:
                if torch.is_tensor(p) and p.numel() >= 4:
                    worst = max(worst, rel_max(p, q))
    return worst


# ------------------------------------------------------------------------------------------------ the cases both test modules run

S_ONE = 4                                   # single launches: a four-index schedule, indices S - 1, 1, 0
IDX_ONE = (S_ONE - 1, 1, 0)
SHAPE_CFG = [(s, cfg) for s in SHAPES for cfg in ((False, True) if s[2] == 0 else (False,))]      # guidance only without concat


def both(fn):
    """(fp32 result, fp64 result) of fn(dt)."""
    return fn(F32), fn(F64)


def prepare_case(shape, cfg, idx, masked, seed=11):
    B, per, per_c = shape
    nB = 2 * B if cfg else B
    d = latent_inputs(B, per, per_c, cfg, S_ONE, seed)
    sch = ddim_schedule(S_ONE, ETA)
    rows = ddim_coef_rows(sch, ddim_log_slots(S_ONE, 2)[0], masked)
    m = dict(mask=d["mask"], x0=d["x0"], z=d["noise_q"][S_ONE - 1 - idx]) if masked else {}
    ref = both(lambda dt: prepare(d["x"], d["concat"], nB, rows[idx], dt, **m))
    return dict(inp=d, sch=sch, rows=rows, nB=nB, ref=ref)


def ddim_case(shape, cfg, idx, noise, slot=-1, seed=12):
    """One DDIM step on the model input prepare builds (no mask); noise: eta > 0 with the step's draw, else sigma = 0 in the slot."""
    B, per, per_c = shape
    nB = 2 * B if cfg else B
    d = latent_inputs(B, per, per_c, cfg, S_ONE, seed)
    sch = ddim_schedule(S_ONE, ETA if noise else 0.0)
    row = ddim_coef_rows(sch, masked=False)[idx].clone()
    row[6] = float(slot)
    xin = prepare(d["x"], d["concat"], nB, row, F32)
    z = d["noise_p"][S_ONE - 1 - idx] if noise else None
    ref = both(lambda dt: ddim_step(xin[:B, :per], d["eu"], d["ec"], SCALE, row, dt, z, TEMPERATURE if noise else None))
    return dict(inp=d, row=row, xin=xin, nB=nB, ref=ref)


def encode_case(B, per, seed=13):
    """stochastic_encode from x0 and from moments, one index per sample; logvar -31, -30, 20, 21 in front so both clamps bind."""
    g = gen(seed)
    sch = ddim_schedule(S_ONE)
    sqrt_a, sqrt_1ma = sqrt(sch["a"]), sqrt(one(F32) - sch["a"])
    t = torch.arange(B) % S_ONE
    x0, noise, n_post = randn(g, B, per), randn(g, B, per), randn(g, B, per)
    moments = randn(g, B, 2, per)
    moments[:, 1, :4] = torch.tensor([-31.0, -30.0, 20.0, 21.0])
    scale_factor = 0.18215
    plain = both(lambda dt: stochastic_encode(x0, t, sqrt_a, sqrt_1ma, noise, dt)[0])
    mom = both(lambda dt: stochastic_encode(None, t, sqrt_a, sqrt_1ma, noise, dt, moments, scale_factor, n_post)[0])
    return dict(x0=x0, noise=noise, n_post=n_post, moments=moments, t=t, sqrt_a=sqrt_a, sqrt_1ma=sqrt_1ma, scale_factor=scale_factor,
                plain=plain, mom=mom)


DDPM_T = 6


def ddpm_update_case(B, per, clip, seed=14):
    """p_sample with one timestep per sample, t[b] = b % T (sample 0 at t = 0, whose draw is NaN: the no-noise row)."""
    g = gen(seed)
    tabs = posterior_tables(DDPM_T)
    rows = ddpm_rows(tabs, TEMPERATURE)
    t = torch.arange(B) % DDPM_T
    x, e, z = randn(g, B, per), randn(g, B, per), randn(g, B, per)
    if clip:
        for b in range(B):
            xb, eb = plant_clamp(x[b:b + 1], e[b:b + 1], rows[int(t[b]), 0])
            x[b], e[b] = xb[0], eb[0]
    z[t == 0] = float("nan")
    def ref(dt):
        out = [ddpm_step(x[b], e[b], z[b], rows[int(t[b])], clip, dt) for b in range(B)]
        return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
    return dict(tabs=tabs, t=t, x=x, e=e, z=z, ref=both(ref))


def ds_update_case(B, per, clip, seed=15):
    g = gen(seed)
    tabs = posterior_tables(DDPM_T)
    rows = ds_rows(tabs)
    t = (torch.arange(B) + 2) % DDPM_T
    x, e, z = randn(g, B, per), randn(g, B, per), randn(g, B, per)
    ref = both(lambda dt: torch.stack([ds_ddpm_step(x[b], e[b], z[b], rows[int(t[b])], clip, dt) for b in range(B)]))
    return dict(tabs=tabs, rows=rows, t=t, x=x, e=e, z=z, ref=ref)


# chained trajectories: name -> (fp32 chain, fp64 chain, inputs)
PLMS_S = 7
DDPM_START = 5
DS_TIMESTEPS = 100
DS_INTERVAL = 10
DS_DDPM_START = 4


@functools.lru_cache(maxsize=None)
def chain_case(name, shape=(2, 40, 0), cfg=False, variant=0):
    """The chained cases of the GPU tests, computed once: dict(c32, c64, model, inputs ...)."""
    B, per, per_c = shape
    nB = 2 * B if cfg else B
    if name in ("ddim", "plms"):
        plms = name == "plms"
        S = PLMS_S if plms else S_ONE
        masked, noisy = variant == 1, variant == 1 and not plms
        d = latent_inputs(B, per, per_c, cfg, S, 21 + variant)
        sch = ddim_schedule(S, ETA if noisy else 0.0)
        slots, n_log = ddim_log_slots(S, 3)
        model = SyntheticModel(nB, per, S + 1, 22)
        kw = dict(concat=d["concat"], slots=slots, plms=plms)
        if masked:
            kw.update(mask=d["mask"], x0=d["x0"], noise_q=d["noise_q"])
        if noisy:
            kw.update(noise_p=d["noise_p"], temperature=TEMPERATURE)
        c32, c64 = both(lambda dt: ddim_chain(model, sch, d["x"], nB, SCALE, dt, **kw))
        return dict(c32=c32, c64=c64, model=model, inp=d, sch=sch, slots=slots, n_log=n_log, S=S, masked=masked, noisy=noisy, nB=nB)
    if name == "ddpm":
        clip, masked = bool(variant & 1), bool(variant & 2)
        T = DDPM_START + 1
        d = latent_inputs(B, per, 0, cfg, T, 31 + variant)
        slots = [0 if t == DDPM_START else (1 + (DDPM_START - t) // 2 if t % 2 == 0 else -1) for t in range(T)]      # t = 5, 4, 2, 0
        tab = ddpm_rows(posterior_tables(T), TEMPERATURE, slots, masked)
        x_T, _ = plant_clamp(d["x"], d["x"], tab[DDPM_START, 0]) if clip else (d["x"], None)
        model = SyntheticModel(nB, per, T, 32)
        if clip:                      # the first evaluation returns 0 on the planted elements: x_recon = c0 x exactly
            model.a = model.a.expand(-1, -1, per).clone()
            model.a[0, :, :4], model.r[0, :, :4] = 0.0, 0.0
        noise_p = d["noise_p"].clone()
        noise_p[DDPM_START] = float("nan")          # the t = 0 draw is not read
        kw = dict(mask=d["mask"], x0=d["x0"], noise_q=d["noise_q"]) if masked else {}
        c32, c64 = both(lambda dt: ddpm_chain(model, tab, x_T, DDPM_START, clip, dt, nB, SCALE, noise_p=noise_p, **kw))
        return dict(c32=c32, c64=c64, model=model, inp=d, tab=tab, x_T=x_T, noise_p=noise_p, clip=clip, masked=masked, nB=nB,
                    n_log=4)
    if name == "ds_plms":
        from oracle import diffsinger as ODS
        t0 = variant
        ac = ODS.alphas_cumprod(DS_TIMESTEPS, 0.06)
        g = gen(41 + t0)
        x_T = randn(g, B, per)
        model = SyntheticModel(B, per, t0 // DS_INTERVAL + 2, 42)
        c32, c64 = both(lambda dt: ds_plms_chain(model, ac, x_T, t0, DS_INTERVAL, dt))
        return dict(c32=c32, c64=c64, model=model, ac=ac, x_T=x_T, t0=t0)
    assert name == "ds_ddpm"
    clip = bool(variant)
    g = gen(51)
    tab = ds_rows(posterior_tables(DS_DDPM_START + 2))
    x_T = randn(g, B, per)
    noise = randn(g, DS_DDPM_START + 1, B, per) + (torch.arange(DS_DDPM_START + 1, dtype=F32) + 1).reshape(-1, 1, 1) * DRAW_OFFSET
    model = SyntheticModel(B, per, DS_DDPM_START + 1, 52)
    c32, c64 = both(lambda dt: ds_ddpm_chain(model, tab, x_T, DS_DDPM_START, clip, noise, dt))
    return dict(c32=c32, c64=c64, model=model, tab=tab, x_T=x_T, noise=noise, clip=clip)


CHAINS = ([("ddim", s, cfg, v) for s, cfg in SHAPE_CFG for v in (0, 1)] + [("plms", s, cfg, v) for s, cfg in SHAPE_CFG for v in (0, 1)] +
          [("ddpm", s, cfg, v) for s, cfg in SHAPE_CFG if s[2] == 0 for v in (0, 1, 2, 3)] +
          [("ds_plms", (2, 40, 0), False, t0) for t0 in (55, 60)] + [("ds_plms", (3, 42, 0), False, 55)] +
          [("ds_ddpm", (2, 40, 0), False, v) for v in (0, 1)])
