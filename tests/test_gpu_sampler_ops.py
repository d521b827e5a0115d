"""The sampling loops' step kernels on their own (csrc/sampler_steps.hip: ddim_* / ldm_plms_* / ddpm_* / ds_plms* / ds_ddpm*),
launched exactly as the loops launch them through maa_op_sampler_step (which forwards every argument of one internal launch and
adds nothing) and through maa_ddim_update, maa_ddim_stochastic_encode, maa_ddpm_update and maa_ds_ddpm_update.

Gates.  Every output is held twice (tests/sampler_ref.py): torch.equal to the fp32 restatement of the reference's lines, one
correctly rounded operation at a time in the reference's term order, and within a rel-max gate of the float64 evaluation of the
same formula: 1e-5 of max|reference| for one launch (the project's elementwise operator gate); for chained launches twice the
distance between the fp32 and the float64 chain on the CPU, computed from the same chains at run time (the device has to equal
the fp32 chain anyway).  Largest fp32-to-float64 distances of the chains used here, measured on the CPU
(tests/test_sampler_ref.py asserts they stay below these): DDIM 2.9e-7 (S = 4), PLMS 1.1e-6 (S = 7), DDPM 1.3e-6 (6 steps),
DiffSinger PLMS 1.7e-7 (7 steps), DiffSinger DDPM 1.4e-7 (5 steps).
The one output not held bit for bit is stochastic_encode from moments: its prologue calls expf, whose device result may differ
from the host's by an ulp; it is gated at 1e-5 against float64 only (measured on the CPU, torch's exp against float64: 6e-8).

The kernels do not depend on the context's precision mode (they contain no contraction); the module runs on one f32 context and
test_ddim_chain_is_the_same_under_bf16x3 shows one chain equal bit for bit under bf16x3.

Every buffer a launch may write has sentinel floats behind it (and one in front of it when it is placed one float off
alignment), inside the same allocation; buffers that must stay untouched are all sentinel.

Finding, not a kernel bug: torch's own fp32 sqrt on the CPU is an ulp off on about one value in six on the device's host (its
add, sub, mul and div are IEEE there), which showed as a 4-ulp difference of one DDIM x_prev; the restatement takes a correctly
rounded sqrt (sampler_ref.sqrt), as the kernels' sqrtf is.  With it every output of every kernel here is bit-equal.

Every case is launched twice with equal bits (the exact expectations of euler_mid, the embedding rows, the guard and the
advance are compared on both launches).

Contracts that differ from the reference, on purpose: at the t = 0 row (sd = 0) ddpm_step_kernel / ddpm_update_kernel do not
read the draw (the reference multiplies it by zero), so a NaN draw gives the mean; with noise_p = NULL the DDIM step adds no
noise whatever sigma the slot holds.

Which case hits which mechanism:
  V = 1 by per % 4 != 0                 shape (3, 42, 0) of every chain, test_ddpm_update, test_stochastic_encode
  V = 1 by per_in % 4 != 0              shape (2, 40, 6) of test_ddim_chain / test_plms_chain
  V = 1 by misalignment                 test_misaligned_*, test_stochastic_encode[misaligned], test_ddpm_update (misaligned)
  second grid-stride trip               test_grid_stride
  ring wrap at order 3                  test_plms_chain steps i = 4, 5, 6 (S = 7)
  a_prev = 1 below interval             test_ds_plms_chain t0 = 55 (t = 5) and t0 = 60 (t = 0)
  log slot -1 / slot k                  test_ddim_step_logs, every chain (log_every_t = 3: unlogged steps in between)
  the t = 0 no-noise row                test_ddpm_chain (NaN draw), test_ddpm_update (sample 0)
  both clamps                           test_ddpm_chain clip (x_recon exactly +-1 and beyond), test_stochastic_encode moments
  guarded out-of-range paths            test_ddpm_update / test_stochastic_encode bad index, test_ds_ddpm_guard,
                                        test_ds_ddpm_update
  emb_w loop with fewer threads         test_prepare_embedding_and_crop_rows (emb_w = 1284, one block)
  n_t > nB                              test_prepare_embedding_and_crop_rows, test_euler_mid_moves_the_timestep
  ds_plms_advance at B = 256, clamp     test_ds_advance
The device helpers two loops share (sampler_steps.hip), each branch from both sides:
  adams_bashforth orders 1, 2, 3        test_ldm_chain[plms] steps i = 1, 2, 3.. (S = 7); test_ds_plms_chain history counts 1, 2, 3..
  posterior_mean clamp on / off         test_ldm_chain[ddpm] variants 1, 3 / 0, 2 and test_ddpm_update; test_ds_ddpm_chain and
                                        test_ds_ddpm_update, clip False / True
  ddim_x_prev scalar and vector         test_ddim_step with maa_ddim_update (V = 1 kernels); test_ldm_chain[plms],
                                        test_euler_mid_moves_the_timestep"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sampler_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
PAD = 8
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def contexts():
    from audiogpt_amd.backend import Context
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = Context(DEV, precision=precision)
        return made[precision]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def ctx(contexts):
    return contexts("f32")


class Buf:
    """n floats (or int32) on the device with PAD sentinels behind them, `off` floats into the allocation (off = 1: one float off
    16-byte alignment, with a sentinel in front)."""

    def __init__(self, n, src=None, off=0, dtype=F32):
        self.n, self.off = int(n), off
        self.all = torch.full((self.n + PAD + 4,), SENTINEL if dtype == F32 else -12345, dtype=dtype, device=DEV)
        self.v = self.all[off:off + self.n]
        assert (self.v.data_ptr() % 16 == 0) == (off % 4 == 0)
        if src is not None:
            self.v.copy_(torch.as_tensor(src).reshape(-1).to(dtype))

    @property
    def ptr(self):
        return self.v.data_ptr() if self.n > 0 else None

    def take(self, *shape):
        t = self.all.cpu()
        inside = torch.zeros(t.shape[0], dtype=torch.bool)
        inside[self.off:self.off + self.n] = True
        assert bool((t[~inside] == self.all.new_tensor(SENTINEL).cpu()).all()), "store outside the buffer"
        v = t[self.off:self.off + self.n]
        return v.reshape(*shape) if shape else v

    def untouched(self):
        return bool((self.take() == SENTINEL).all())


def close(name, dev, ref32, ref64, gate, exact=True):
    """dev equals the fp32 reference bit for bit (values: -0 == +0) and is within `gate` of the float64 one."""
    dev, ref32 = dev.reshape(-1), ref32.reshape(-1)
    if exact:
        bad = (dev != ref32).nonzero().reshape(-1)
        assert bad.numel() == 0, "%s: %d of %d elements differ from the fp32 restatement, first at %d: %r vs %r" % (
            name, bad.numel(), dev.numel(), int(bad[0]), float(dev[bad[0]]), float(ref32[bad[0]]))
    d = R.rel_max(dev, ref64.reshape(-1))
    print("%s: rel-max to float64 %.3g (gate %.3g)" % (name, d, gate))
    assert d <= gate, "%s: %.3g of max|ref| from float64, gate %.3g" % (name, d, gate)


# ---------------------------------------------------------------------------------------------------- the ldm loops' buffers

class Rig:
    """The device state of one DDIM / PLMS / DDPM loop as the caller of maa_op_sampler_step owns it."""

    def __init__(self, ctx, shape, nB, S, x, concat=None, tab_t=None, rows=None, n_log=0, mask=None, x0=None, noise_q=None,
                 noise_p=None, dtab=None, emb_w=0, n_t=0, mis=(), start=0, clip=0, temperature=1.0):
        self.ctx = ctx
        self.B, self.per, per_c = shape
        self.nB, self.S, self.per_in, self.n = nB, S, self.per + per_c, self.B * self.per
        self.n_log, self.emb_w, self.n_t, self.start, self.clip, self.temperature = n_log, emb_w, n_t, start, clip, temperature
        off = lambda name: 1 if name in mis else 0
        n = self.n
        b = self.b = {}
        b["x"] = Buf(n, x, off("x"))
        b["concat"] = Buf(self.B * per_c, concat)
        b["xin"] = Buf(nB * self.per_in, None, off("xin"))
        b["eps"] = Buf(nB * self.per, None, off("eps"))
        b["coef"], b["cur_t"] = Buf(8), Buf(n_t if n_t > 0 else nB)
        b["tab_t"], b["tab"] = Buf(S, tab_t), Buf(S * 8, rows)
        b["ring"] = Buf(3 * n, None, off("ring"))
        b["log_x"], b["log_x0"] = Buf(n_log * n), Buf(n_log * n)
        for name, src in (("mask", mask), ("x0", x0), ("noise_q", noise_q), ("noise_p", noise_p), ("dtab", dtab)):
            b[name] = Buf(src.numel() if src is not None else 0, src)
        g = R.gen(77)
        self.emb_tab = R.randn(g, S, emb_w) if emb_w else None
        b["emb_tab"], b["cur_emb"] = Buf(S * emb_w, self.emb_tab), Buf(emb_w)
        self.step = Buf(1, dtype=torch.int32)
        self.logged = {}                      # slot -> (x, x0) expected so far
        self.ring_seen = [None, None, None]

    def set_step(self, idx):
        self.step.v.fill_(idx)

    def launch(self, kind, **over):
        b = self.b
        f = dict(B=self.B, nB=self.nB, S=self.S, n=self.n, per=self.per, per_in=self.per_in, scale=R.SCALE,
                 temperature=self.temperature, start=self.start, clip=self.clip, emb_w=self.emb_w, n_t=self.n_t,
                 d_x=b["x"].ptr, d_concat=b["concat"].ptr, d_xin=b["xin"].ptr, d_eps_u=b["eps"].ptr,
                 d_eps_c=b["eps"].v[self.n:].data_ptr() if self.nB > self.B else None, d_coef=b["coef"].ptr,
                 d_tab_t=b["tab_t"].ptr, d_tab=b["dtab"].ptr if kind == "ddpm" else b["tab"].ptr, d_step=self.step.v.data_ptr(),
                 d_cur_t=b["cur_t"].ptr, d_emb_tab=b["emb_tab"].ptr, d_cur_emb=b["cur_emb"].ptr, d_mask=b["mask"].ptr,
                 d_x0=b["x0"].ptr, d_noise_q=b["noise_q"].ptr, d_noise_p=b["noise_p"].ptr, d_ring=b["ring"].ptr,
                 d_e_keep=b["ring"].ptr, d_log_x=b["log_x"].ptr, d_log_x0=b["log_x0"].ptr)
        f.update(over)
        self.ctx.op_sampler_step(kind, **f)

    def evaluate(self, model, k):
        """eps = a_k * x + b_k * randn_k on the latent channels of the step's model input, by torch on the device in fp32."""
        a, bk, r = (t.to(DEV) for t in model.terms(k))
        xin = self.b["xin"].v.reshape(self.nB, self.per_in)[:, :self.per]
        self.b["eps"].v.copy_((a * xin + bk * r).reshape(-1))

    def check(self, name, e32, e64, gate):
        """The buffers a launch leaves, against the expectations of the two chains; returns what was read back."""
        B, per, n = self.B, self.per, self.n
        got = []
        for key, v in e32.items():
            w = e64[key]
            if key == "xin":
                t = self.b["xin"].take(self.nB, self.per_in)
                close(name + " xin", t, v, w, gate)
            elif key == "coef":
                t = self.b["coef"].take()
                assert torch.equal(t, v), (name, t, v)
            elif key == "cur_t":
                t = self.b["cur_t"].take()
                assert bool((t == v).all()), (name, t, v)
            elif key == "step":
                t = self.step.take()
                assert int(t[0]) == v, (name, t, v)
            elif key == "x":
                t = self.b["x"].take(B, per)
                close(name + " x", t, v, w, gate)
            elif key == "ring":
                t = self.b["ring"].take(3, B, per)
                for s in range(3):
                    if v[s] is None:
                        assert bool((t[s] == SENTINEL).all()), "%s: ring slab %d written" % (name, s)
                    else:
                        close("%s ring[%d]" % (name, s), t[s], v[s], w[s], gate)
            elif key == "log_x":
                self.logged[v[0]] = (v[1], e32["log_x0"][1], w[1], e64["log_x0"][1])
                continue
            else:
                continue
            got.append(t)
        if self.n_log:
            lx, l0 = self.b["log_x"].take(self.n_log, B, per), self.b["log_x0"].take(self.n_log, B, per)
            for s in range(self.n_log):
                if s in self.logged:
                    close("%s log_x[%d]" % (name, s), lx[s], self.logged[s][0], self.logged[s][2], gate)
                    close("%s log_x0[%d]" % (name, s), l0[s], self.logged[s][1], self.logged[s][3], gate)
                else:
                    assert bool((lx[s] == SENTINEL).all() and (l0[s] == SENTINEL).all()), "%s: log slab %d written early" % (name, s)
            got += [lx, l0]
        return got


def run_ldm_chain(ctx, name, shape, cfg, variant, mis=(), logs=True):
    """One chained case of sampler_ref.chain_case on the device, compared after every launch; returns everything read back."""
    k = R.chain_case(name, shape, cfg, variant)
    gate = 2 * R.chain_distance(k["c32"], k["c64"])
    d = k["inp"]
    if name == "ddpm":
        T = k["tab"].shape[0]
        rig = Rig(ctx, shape, k["nB"], T, k["x_T"], None, torch.arange(T, dtype=F32), R.identity_coef_rows(T), k["n_log"] if logs else 0,
                  d["mask"] if k["masked"] else None, d["x0"] if k["masked"] else None, d["noise_q"] if k["masked"] else None,
                  k["noise_p"], k["tab"], mis=mis, start=R.DDPM_START, clip=int(k["clip"]))
        rig.set_step(R.DDPM_START)
    else:
        S, sch = k["S"], k["sch"]
        rig = Rig(ctx, shape, k["nB"], S, d["x"], d["concat"], torch.tensor(sch["steps"], dtype=F32),
                  R.ddim_coef_rows(sch, k["slots"], k["masked"]), k["n_log"] if logs else 0,
                  d["mask"] if k["masked"] else None, d["x0"] if k["masked"] else None, d["noise_q"] if k["masked"] else None,
                  d["noise_p"] if k["noisy"] else None, mis=mis, temperature=R.TEMPERATURE if k["noisy"] else 1.0)
        rig.set_step(S - 1)
    got = []
    for i, (l32, l64) in enumerate(zip(k["c32"], k["c64"])):
        if l32["eval"] is not None:
            rig.evaluate(k["model"], l32["eval"])
        over = {}
        if l32["kind"] == "ddim_prepare" and name == "ddpm":
            over = dict(d_mask=None, d_x0=None, d_noise_q=None)          # the ancestral loop blends after the step
        rig.launch(l32["kind"], **over)
        got += rig.check("%s %s %d %s(idx %d)" % (name, shape, i, l32["kind"], l32["idx"]), l32["expect"], l64["expect"], gate)
    for key in ("concat", "tab_t", "tab", "mask", "x0", "noise_q", "noise_p", "dtab", "emb_tab", "cur_emb", "eps"):
        rig.b[key].take()                                                  # nothing stored around the inputs
    return got


def same(a, b):
    assert len(a) == len(b) and all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


CHAIN_IDS = ["%s-B%d-per%d-c%d-%s-v%d" % (n, s[0], s[1], s[2], "cfg" if cfg else "plain", v) for n, s, cfg, v in R.CHAINS]


@pytest.mark.parametrize("name,shape,cfg,variant", [c for c in R.CHAINS if c[0] in ("ddim", "plms", "ddpm")],
                         ids=[i for c, i in zip(R.CHAINS, CHAIN_IDS) if c[0] in ("ddim", "plms", "ddpm")])
def test_ldm_chain(ctx, name, shape, cfg, variant):
    """DDIM (S = 4; variant 1: mask, eta > 0 with temperature 0.7), PLMS (S = 7: Euler pair, orders 1, 2, 3 and three wrapped
    order-3 steps; variant 1: mask) and DDPM (t = 5 .. 0; variant bit 0: clip, bit 1: mask) through PREPARE + the step launches,
    every buffer compared after every launch, logs with log_every_t = 3; launched twice."""
    first = run_ldm_chain(ctx, name, shape, cfg, variant)
    same(first, run_ldm_chain(ctx, name, shape, cfg, variant))


def test_ddim_chain_is_the_same_under_bf16x3(contexts):
    a = run_ldm_chain(contexts("f32"), "ddim", (2, 40, 0), True, 1)
    same(a, run_ldm_chain(contexts("bf16x3"), "ddim", (2, 40, 0), True, 1))


@pytest.mark.parametrize("name,mis", [("ddim", "eps"), ("plms", "eps"), ("plms", "x"), ("ddpm", "eps"), ("ddpm", "x")])
def test_misaligned_chain(ctx, name, mis):
    """(2, 40, 0) once more with eps, or the output latent, one float off alignment (the al16 fallbacks to V = 1): the same bits
    as the aligned call."""
    variant = 3 if name == "ddpm" else 1
    same(run_ldm_chain(ctx, name, (2, 40, 0), True, variant), run_ldm_chain(ctx, name, (2, 40, 0), True, variant, mis=(mis,)))


# ---------------------------------------------------------------------------------------------------- DDIM_PREPARE

@pytest.mark.parametrize("shape,cfg", R.SHAPE_CFG)
@pytest.mark.parametrize("masked", (False, True))
def test_prepare(ctx, shape, cfg, masked):
    """idx in {S - 1, 1, 0}, S = 4: xin rows (latent then concat, the guidance duplicate), the blend with draw S - 1 - idx, cur_t,
    cur_coef; without an embedding table cur_emb is untouched."""
    for idx in R.IDX_ONE:
        k = R.prepare_case(shape, cfg, idx, masked)
        d, sch = k["inp"], k["sch"]
        outs = []
        for _ in range(2):
            rig = Rig(ctx, shape, k["nB"], R.S_ONE, d["x"], d["concat"], torch.tensor(sch["steps"], dtype=F32), k["rows"],
                      mask=d["mask"] if masked else None, x0=d["x0"] if masked else None, noise_q=d["noise_q"] if masked else None)
            cur_emb = Buf(16)
            rig.set_step(idx)
            rig.launch("ddim_prepare", d_cur_emb=cur_emb.ptr)
            name = "prepare %s cfg=%d idx=%d masked=%d" % (shape, cfg, idx, masked)
            e = dict(xin=None, coef=k["rows"][idx], cur_t=float(sch["steps"][idx]), step=idx)
            outs.append(rig.check(name, dict(e, xin=k["ref"][0]), dict(e, xin=k["ref"][1]), R.TOL))
            assert cur_emb.untouched() and rig.b["x"].take().equal(d["x"].reshape(-1))
            if cfg:
                xin = outs[-1][0]
                assert torch.equal(xin[shape[0]:], xin[:shape[0]]), "row b + B differs from row b"
        same(*outs)


def test_prepare_embedding_and_crop_rows(ctx):
    """emb_w = 1284 on (1, 4, 0): one block, five full trips of the embedding loop and a partial sixth; n_t = 3 nB timestep slots (crop rows)."""
    shape = (1, 4, 0)
    for cfg in (False, True, False, True):          # (each twice)
        for idx in R.IDX_ONE:
            k = R.prepare_case(shape, cfg, idx, False)
            nB = k["nB"]
            rig = Rig(ctx, shape, nB, R.S_ONE, k["inp"]["x"], None, torch.tensor(k["sch"]["steps"], dtype=F32), k["rows"],
                      emb_w=R.EMB_W, n_t=3 * nB)
            rig.set_step(idx)
            rig.launch("ddim_prepare")
            e = dict(xin=k["ref"][0], coef=k["rows"][idx], cur_t=float(k["sch"]["steps"][idx]))
            rig.check("prepare emb idx=%d" % idx, e, dict(e, xin=k["ref"][1]), R.TOL)
            assert rig.b["cur_t"].n == 3 * nB
            assert torch.equal(rig.b["cur_emb"].take(), rig.emb_tab[idx]), "cur_emb is not row idx of the table"


# ---------------------------------------------------------------------------------------------------- DDIM

def ddim_rig(ctx, shape, k, noise, n_log=0):
    d = k["inp"]
    rig = Rig(ctx, shape, k["nB"], R.S_ONE, None, None, n_log=n_log, noise_p=d["noise_p"] if noise else None,
              temperature=R.TEMPERATURE)
    rig.b["xin"].v.copy_(k["xin"].reshape(-1))
    rig.b["coef"].v.copy_(k["row"])
    rig.b["eps"].v[:rig.n].copy_(d["eu"].reshape(-1))
    if d["ec"] is not None:
        rig.b["eps"].v[rig.n:].copy_(d["ec"].reshape(-1))
    return rig


@pytest.mark.parametrize("shape,cfg", R.SHAPE_CFG)
@pytest.mark.parametrize("noise", (False, True))
def test_ddim_step(ctx, shape, cfg, noise):
    """x from the first B rows of xin at pitch per_in, with and without ec, eta > 0 with temperature 0.7 and draw S - 1 - idx,
    *step = idx - 1 (-1 after idx = 0); maa_ddim_update on the same inputs gives the same bits, in place too."""
    B, per, _ = shape
    for idx in R.IDX_ONE:
        k = R.ddim_case(shape, cfg, idx, noise)
        (x32, p32), (x64, p64) = k["ref"]
        name = "ddim %s cfg=%d idx=%d noise=%d" % (shape, cfg, idx, noise)
        outs = []
        for _ in range(2):
            rig = ddim_rig(ctx, shape, k, noise)
            rig.step.v.fill_(99)
            rig.launch("ddim", d_log_x=None, d_log_x0=None)
            outs.append(rig.check(name, dict(x=x32, step=idx - 1), dict(x=x64, step=idx - 1), R.TOL))
            assert torch.equal(rig.b["xin"].take(), k["xin"].reshape(-1)) and rig.b["ring"].untouched()
        same(*outs)
        if not noise and shape[2] == 0:          # maa_ddim_update: the same arithmetic on a plain latent, out of place and in place
            d = k["inp"]
            x, xp, pred = Buf(B * per, d["x"]), Buf(B * per), Buf(B * per)
            coef = Buf(4, k["row"][:4])
            eu, ec = Buf(B * per, d["eu"]), Buf(B * per, d["ec"]) if cfg else None
            args = (eu.ptr, ec.ptr if cfg else None, float(R.SCALE), coef.ptr, B * per)
            ctx._call("maa_ddim_update", x.ptr, *args, xp.ptr, pred.ptr)
            torch.cuda.synchronize()
            close(name + " update x_prev", xp.take(), x32, x64, R.TOL)
            close(name + " update pred_x0", pred.take(), p32, p64, R.TOL)
            ctx._call("maa_ddim_update", x.ptr, *args, x.ptr, None)
            torch.cuda.synchronize()
            close(name + " update in place", x.take(), x32, x64, R.TOL)


def test_ddim_step_without_noise_buffer_adds_no_noise(ctx):
    """noise_p = NULL with sigma > 0 in the slot: the noise term is not formed."""
    shape = (2, 40, 0)
    k = R.ddim_case(shape, True, 1, True)
    ref = R.both(lambda dt: R.ddim_step(k["xin"][:2, :40], k["inp"]["eu"], k["inp"]["ec"], R.SCALE, k["row"], dt))
    assert float(k["row"][2]) > 0
    outs = []
    for _ in range(2):
        rig = ddim_rig(ctx, shape, k, False)
        rig.launch("ddim", d_log_x=None, d_log_x0=None)
        outs.append(rig.check("ddim no noise buffer", dict(x=ref[0][0]), dict(x=ref[1][0]), R.TOL))
    same(*outs)


def test_ddim_step_logs(ctx):
    """slot -1 writes nothing; slot k writes slab k of both logs and no other; log_x = NULL with a slot >= 0 is safe."""
    shape = (2, 40, 0)
    for slot in (-1, 0, 2):
        k = R.ddim_case(shape, False, 1, True, slot)
        (x32, p32), (x64, p64) = k["ref"]
        e32, e64 = dict(x=x32), dict(x=x64)
        if slot >= 0:
            e32.update(log_x=(slot, x32), log_x0=(slot, p32))
            e64.update(log_x=(slot, x64), log_x0=(slot, p64))
        outs = []
        for _ in range(2):
            rig = ddim_rig(ctx, shape, k, True, n_log=3)
            rig.launch("ddim")
            outs.append(rig.check("ddim logs slot=%d" % slot, e32, e64, R.TOL))
        same(*outs)
        rig = ddim_rig(ctx, shape, k, True, n_log=3)
        rig.launch("ddim", d_log_x=None, d_log_x0=None)
        rig.check("ddim null logs slot=%d" % slot, dict(x=x32), dict(x=x64), R.TOL)


# ---------------------------------------------------------------------------------------------------- PLMS pieces

def test_euler_mid_moves_the_timestep(ctx):
    """EULER_MID moves cur_t (n_t = 3 nB slots) and cur_emb to tab_t[max(idx - 1, 0)]: idx = 2 -> 1 and, as at S = 1, idx = 0 -> 0;
    the concat channels of xin survive and both guidance halves get x_mid (test_ldm_chain compares xin whole)."""
    shape = (2, 40, 0)
    for idx in (2, 0, 2, 0):          # (each twice)
        k = R.prepare_case(shape, True, idx, False)
        nB = k["nB"]
        rig = Rig(ctx, shape, nB, R.S_ONE, k["inp"]["x"], None, torch.tensor(k["sch"]["steps"], dtype=F32), k["rows"],
                  emb_w=R.EMB_W, n_t=3 * nB)
        rig.set_step(idx)
        rig.launch("ddim_prepare")
        rig.b["eps"].v.copy_(torch.cat([k["inp"]["eu"], k["inp"]["ec"]]).reshape(-1))
        rig.launch("plms_euler_mid")
        nxt = max(idx - 1, 0)
        assert bool((rig.b["cur_t"].take() == float(k["sch"]["steps"][nxt])).all())
        assert torch.equal(rig.b["cur_emb"].take(), rig.emb_tab[nxt])
        assert int(rig.step.take()[0]) == idx, "EULER_MID moved the step index"
        xin = rig.b["xin"].take(nB, 40)
        assert torch.equal(xin[:2], xin[2:])
        x_mid = R.both(lambda dt: R.x_prev_and_pred_x0(k["ref"][0][:2], R.cfg_eps(k["inp"]["eu"], k["inp"]["ec"], R.SCALE, dt),
                                                       k["rows"][idx], dt)[0])
        close("euler_mid idx=%d" % idx, xin[:2], x_mid[0], x_mid[1], R.TOL)


# ---------------------------------------------------------------------------------------------------- grid stride

@pytest.mark.parametrize("kind", ("ddim", "plms", "ddpm"))
@pytest.mark.parametrize("B,per", R.GRID_SHAPES)
def test_grid_stride(ctx, kind, B, per):
    """More vectors (V = 4: per = 4 194 312, B = 2) or elements (V = 1: per = 2 097 153) than 8192 blocks of 256 threads hold:
    the loops go round again.  Against the fp32 restatement only; no mask, no logs."""
    n = B * per
    g = R.gen(61)
    x, e, z = R.randn(g, B, per), R.randn(g, B, per), R.randn(g, B, per)
    S = 5
    sch = R.ddim_schedule(S)
    row = R.ddim_coef_rows(sch, masked=False)[1]            # idx = 1: PLMS step i = 3, order 3
    ring_src = R.randn(g, 3, B, per)
    tab = R.ddpm_rows(R.posterior_tables(S), R.TEMPERATURE, masked=False)
    outs = []
    for _ in range(2):
        xin, eps, out, coef, step = Buf(n, x), Buf(n, e), Buf(n), Buf(8, row), Buf(1, dtype=torch.int32)
        f = dict(B=B, nB=B, S=S, n=n, per=per, per_in=per, scale=1.0, temperature=1.0, d_x=out.ptr, d_xin=xin.ptr, d_eps_u=eps.ptr,
                 d_coef=coef.ptr, d_step=step.v.data_ptr())
        if kind == "ddim":
            ctx.op_sampler_step("ddim", **f)
            ref = R.ddim_step_f32(x, e, None, 1.0, row)[0]
        elif kind == "plms":
            ring = Buf(3 * n, ring_src)
            ctx.op_sampler_step("plms", d_ring=ring.ptr, **f)
            w, h1, h2, h3 = R.ring_slots(S - 1 - 1)
            ref = R.x_prev_and_pred_x0_f32(x, R.plms_e_prime(e, [ring_src[h3], ring_src[h2], ring_src[h1]], F32), row)[0]
            got = ring.take(3, B, per)
            assert torch.equal(got[w], e) and torch.equal(got[h1], ring_src[h1]) and torch.equal(got[h2], ring_src[h2])
        else:
            noise, dtab = Buf(n, z), Buf(tab.numel(), tab)
            ctx.op_sampler_step("ddpm", d_tab=dtab.ptr, d_noise_p=noise.ptr, start=1, clip=1, **f)
            ref = R.ddpm_step_f32(x, e, z, tab[1], True)[0]
        got = out.take(B, per)
        assert torch.equal(got, ref), "%s: %d elements differ" % (kind, int((got != ref).sum()))
        assert int(step.take()[0]) == 0
        outs.append([got])
    same(*outs)


# ---------------------------------------------------------------------------------------------------- maa_ddpm_update

def call_ddpm_update(ctx, k, t, clip, x, e, z, xp, xr):
    tabs = [k["tabs"][n].numpy() for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1",
                                           "posterior_mean_coef2", "posterior_log_variance_clipped")]
    fp = C.POINTER(C.c_float)
    td = torch.as_tensor(t, dtype=torch.int32).to(DEV)
    B, per = k["x"].shape
    ctx._call("maa_ddpm_update", x.ptr, e.ptr, C.c_void_p(td.data_ptr()), *[a.ctypes.data_as(fp) for a in tabs], R.DDPM_T, z.ptr,
              float(R.TEMPERATURE), int(clip), B, 1, 1, per, xp.ptr, xr.ptr)


@pytest.mark.parametrize("B,per", [(6, 40), (7, 42)])
@pytest.mark.parametrize("clip", (False, True))
def test_ddpm_update(ctx, B, per, clip):
    """One timestep per sample, each in range, t = 0 among them (its NaN draw is not read); V = 4, V = 1 by per, V = 1 by a
    misaligned output; clip with x_recon exactly on +-1 and beyond; then t[b] = -1 and t[b] = n_tab: the bad flag is raised and
    that sample alone is zero."""
    from audiogpt_amd._lib import MaaError
    k = R.ddpm_update_case(B, per, clip)
    (xp32, xr32), (xp64, xr64) = k["ref"]
    if clip:
        assert bool((xr32[:, :2].abs() == 1.0).all())
    name = "ddpm_update B%d per%d clip=%d" % (B, per, clip)
    outs = []
    for off in (0, 0, 1):
        x, e, z, xp, xr = Buf(B * per, k["x"]), Buf(B * per, k["e"]), Buf(B * per, k["z"]), Buf(B * per, None, off), Buf(B * per)
        call_ddpm_update(ctx, k, k["t"], clip, x, e, z, xp, xr)
        got = [xp.take(B, per), xr.take(B, per)]
        close(name + " x_prev", got[0], xp32, xp64, R.TOL)
        close(name + " x_recon", got[1], xr32, xr64, R.TOL)
        assert bool(torch.isfinite(got[0]).all())
        outs.append(got)
    same(outs[0], outs[1])
    same(outs[0], outs[2])
    for bad in (-1, R.DDPM_T):
        t = k["t"].clone()
        t[1] = bad
        x, e, z, xp, xr = Buf(B * per, k["x"]), Buf(B * per, k["e"]), Buf(B * per, k["z"]), Buf(B * per), Buf(B * per)
        with pytest.raises(MaaError, match="outside"):
            call_ddpm_update(ctx, k, t, clip, x, e, z, xp, xr)
        got = xp.take(B, per)
        keep = torch.arange(B) != 1
        assert bool((got[1] == 0).all() and (xr.take(B, per)[1] == 0).all()) and torch.equal(got[keep], xp32[keep])


# ---------------------------------------------------------------------------------------------------- stochastic encode

@pytest.mark.parametrize("B,per,off", [(4, 40, 0), (3, 42, 0), (4, 40, 1)], ids=["v4", "v1", "misaligned"])
def test_stochastic_encode(ctx, B, per, off):
    """From x0 (bit for bit) and from moments with logvar -31, -30, 20, 21 (both clamps bind; expf: float64 gate only), one index per
    sample; then a bad index: the flag is raised and that sample alone is zero."""
    from audiogpt_amd._lib import MaaError
    k = R.encode_case(B, per)
    fp = C.POINTER(C.c_float)
    sa, sb = k["sqrt_a"].numpy(), k["sqrt_1ma"].numpy()

    def call(src, moments, t, out, n_post):
        td = torch.as_tensor(t, dtype=torch.int32).to(DEV)
        ctx._call("maa_ddim_stochastic_encode", src.ptr, int(moments), float(k["scale_factor"]), n_post.ptr if n_post else None,
                  C.c_void_p(td.data_ptr()), sa.ctypes.data_as(fp), sb.ctypes.data_as(fp), R.S_ONE, noise.ptr, B, 1, 1, per, out.ptr)

    outs = []
    for _ in range(2):
        noise, x0, out = Buf(B * per, k["noise"]), Buf(B * per, k["x0"]), Buf(B * per, None, off)
        call(x0, False, k["t"], out, None)
        got = [out.take(B, per)]
        close("encode x0 B%d per%d off%d" % (B, per, off), got[0], k["plain"][0], k["plain"][1], R.TOL)
        mom, n_post, out = Buf(B * 2 * per, k["moments"]), Buf(B * per, k["n_post"]), Buf(B * per, None, off)
        call(mom, True, k["t"], out, n_post)
        got.append(out.take(B, per))
        close("encode moments B%d per%d off%d" % (B, per, off), got[1], k["mom"][0], k["mom"][1], R.TOL, exact=False)
        outs.append(got)
    same(*outs)
    for bad in (-1, R.S_ONE):
        t = k["t"].clone()
        t[1] = bad
        noise, x0, out = Buf(B * per, k["noise"]), Buf(B * per, k["x0"]), Buf(B * per, None, off)
        with pytest.raises(MaaError, match="outside"):
            call(x0, False, t, out, None)
        got = out.take(B, per)
        keep = torch.arange(B) != 1
        assert bool((got[1] == 0).all()) and torch.equal(got[keep], k["plain"][0][keep])


# ---------------------------------------------------------------------------------------------------- DiffSinger

class DsRig:
    def __init__(self, ctx, B, per, x, table, st, noise=None, mis=()):
        self.ctx, self.B, self.per, self.n = ctx, B, per, B * per
        n = self.n
        off = lambda name: 1 if name in mis else 0
        self.x, self.x_out, self.e, self.e2 = Buf(n, x), Buf(n), Buf(n, None, off("e")), Buf(n)
        self.hist, self.tab, self.t_slot = Buf(3 * n), Buf(table.numel(), table), Buf(B)
        self.st = Buf(3, torch.tensor(st), dtype=torch.int32)
        self.noise = Buf(noise.numel() if noise is not None else 0, noise)

    def evaluate(self, model, k, on, into):
        a, bk, r = (t.to(DEV) for t in model.terms(k))
        into.v.copy_((a * on.v.reshape(self.B, self.per) + bk * r).reshape(-1))

    def check(self, name, e32, e64, gate):
        B, per = self.B, self.per
        got = [self.x.take(B, per)]
        close(name + " x", got[0], e32["x"], e64["x"], gate)
        st = self.st.take()
        assert st.tolist() == e32["st"], (name, st.tolist(), e32["st"])
        if "x_out" in e32:
            got.append(self.x_out.take(B, per))
            close(name + " x_out", got[-1], e32["x_out"], e64["x_out"], gate)
        if "hist" in e32:
            h = self.hist.take(3, B, per)
            for s in range(3):
                if e32["hist"][s] is None:
                    assert bool((h[s] == SENTINEL).all()), "%s: history slab %d written" % (name, s)
                else:
                    close("%s hist[%d]" % (name, s), h[s], e32["hist"][s], e64["hist"][s], gate)
            got.append(h)
        if "t_slot" in e32:
            t = self.t_slot.take()
            assert bool((t == e32["t_slot"]).all()), (name, t, e32["t_slot"])
        return got


def run_ds_plms_chain(ctx, shape, t0, mis=()):
    k = R.chain_case("ds_plms", shape, False, t0)
    gate = 2 * R.chain_distance(k["c32"], k["c64"])
    B, per, _ = shape
    rig = DsRig(ctx, B, per, k["x_T"], k["ac"], [t0, 0, 0], mis=mis)
    got = []
    for i, (l32, l64) in enumerate(zip(k["c32"], k["c64"])):
        f = dict(B=B, n=rig.n, interval=R.DS_INTERVAL, d_x=rig.x.ptr, d_eps_u=rig.e.ptr, d_ring=rig.hist.ptr, d_tab=rig.tab.ptr,
                 d_st=rig.st.v.data_ptr(), d_cur_t=rig.t_slot.ptr)
        if l32["kind"] == "ds_advance":
            ctx.op_sampler_step("ds_advance", **f)
        else:
            mode = l32["mode"]
            if mode == 2:
                rig.evaluate(k["model"], l32["eval"], rig.x_out, rig.e2)
                f.update(d_eps_u=rig.e.ptr, d_e_prev=rig.e2.ptr)
            else:
                rig.evaluate(k["model"], l32["eval"], rig.x, rig.e)
            if mode == 1:
                f.update(d_x_out=rig.x_out.ptr)
            ctx.op_sampler_step("ds_plms", mode=mode, **f)
        got += rig.check("ds_plms t0=%d %d %s" % (t0, i, l32["kind"]), l32["expect"], l64["expect"], gate)
    rig.tab.take(), rig.e.take(), rig.e2.take()
    return got


@pytest.mark.parametrize("shape,t0", [((2, 40, 0), 55), ((2, 40, 0), 60), ((3, 42, 0), 55)])
def test_ds_plms_chain(ctx, shape, t0):
    """Modes 1, 2, ADVANCE, then mode 0 with ADVANCE: t0 = 55 -> 55, 45, .., 5 (a_prev = 1 below the interval, the last ADVANCE
    clamps a negative t into the slot), t0 = 60 -> .., 0; history counts 1 .. 5 (6) with the ring wrapping.  x, the three history
    slabs, st and the timestep slot after every launch; mode 1 writes x_out only."""
    first = run_ds_plms_chain(ctx, shape, t0)
    same(first, run_ds_plms_chain(ctx, shape, t0))
    if shape[1] % 4 == 0:
        same(first, run_ds_plms_chain(ctx, shape, t0, mis=("e",)))


@pytest.mark.parametrize("B", (1, 3, 256))
def test_ds_advance(ctx, B):
    """t_slot[0 .. B) written and nothing behind it, max(tn, 0) when the next t is negative, st = {tn, cnt + 1, (head + 1) % 3}."""
    for t, interval, cnt, head in ((55, 10, 0, 0), (5, 10, 4, 2), (0, 1, 7, 1)):
        st, slot = Buf(3, torch.tensor([t, cnt, head]), dtype=torch.int32), Buf(B)
        for rep in range(2):
            ctx.op_sampler_step("ds_advance", B=B, interval=interval, d_st=st.v.data_ptr(), d_cur_t=slot.ptr)
            tn = t - interval * (rep + 1)
            assert st.take().tolist() == [tn, cnt + rep + 1, (head + rep + 1) % 3]
            assert bool((slot.take() == float(max(tn, 0))).all())


def run_ds_ddpm_chain(ctx, clip):
    k = R.chain_case("ds_ddpm", (2, 40, 0), False, int(clip))
    gate = 2 * R.chain_distance(k["c32"], k["c64"])
    B, per = 2, 40
    rig = DsRig(ctx, B, per, k["x_T"], k["tab"], [R.DS_DDPM_START, 0, 0], noise=k["noise"])
    got = []
    for i, (l32, l64) in enumerate(zip(k["c32"], k["c64"])):
        if l32["kind"] == "ds_advance":
            ctx.op_sampler_step("ds_advance", B=B, interval=1, d_st=rig.st.v.data_ptr(), d_cur_t=rig.t_slot.ptr)
        else:
            rig.evaluate(k["model"], l32["eval"], rig.x, rig.e)
            ctx.op_sampler_step("ds_ddpm", n=rig.n, d_x=rig.x.ptr, d_eps_u=rig.e.ptr, d_noise_p=rig.noise.ptr, d_tab=rig.tab.ptr,
                                d_st=rig.st.v.data_ptr(), timesteps=k["tab"].shape[0], start=R.DS_DDPM_START,
                                n_steps=R.DS_DDPM_START + 1, clip=int(clip))
        got += rig.check("ds_ddpm clip=%d %d %s" % (clip, i, l32["kind"]), l32["expect"], l64["expect"], gate)
    rig.noise.take(), rig.tab.take()
    assert rig.hist.untouched() and rig.x_out.untouched()
    return got


@pytest.mark.parametrize("clip", (False, True))
def test_ds_ddpm_chain(ctx, clip):
    """t = 4 .. 0 with draw start - t of the call's noise, advance with interval 1 in between."""
    same(run_ds_ddpm_chain(ctx, clip), run_ds_ddpm_chain(ctx, clip))


def test_ds_ddpm_guard(ctx):
    """st[0] = -1, st[0] = timesteps, k = start - t negative, k = n_steps: x is left untouched bit for bit."""
    k = R.chain_case("ds_ddpm", (2, 40, 0), False, 0)
    T = k["tab"].shape[0]
    for t, start, n_steps in ((-1, 4, 5), (T, T, 5), (4, 3, 5), (1, 4, 3)) * 2:
        rig = DsRig(ctx, 2, 40, k["x_T"], k["tab"], [t, 0, 0], noise=k["noise"])
        rig.e.v.copy_(k["noise"][0].reshape(-1))
        ctx.op_sampler_step("ds_ddpm", n=rig.n, d_x=rig.x.ptr, d_eps_u=rig.e.ptr, d_noise_p=rig.noise.ptr, d_tab=rig.tab.ptr,
                            d_st=rig.st.v.data_ptr(), timesteps=T, start=start, n_steps=n_steps, clip=1)
        assert torch.equal(rig.x.take(2, 40).view(torch.int32), k["x_T"].view(torch.int32)), (t, start, n_steps)
        assert rig.st.take().tolist() == [t, 0, 0]


@pytest.mark.parametrize("clip", (False, True))
def test_ds_ddpm_update(ctx, clip):
    """maa_ds_ddpm_update with one float t per sample: every sample in range is updated with its own row (t[b] = 2.0 with row 2);
    t[b] in {-1.0, timesteps, NaN}: sample b unchanged, the bad flag raised."""
    from audiogpt_amd._lib import MaaError
    B, per = 6, 40
    k = R.ds_update_case(B, per, clip)
    fp = C.POINTER(C.c_float)
    cols = [np.ascontiguousarray(k["rows"][:, j].numpy()) for j in range(5)]

    def call(t, x, e, z):
        td = torch.as_tensor(t, dtype=F32).to(DEV)
        ctx._call("maa_ds_ddpm_update", e.ptr, C.c_void_p(td.data_ptr()), z.ptr, *[c.ctypes.data_as(fp) for c in cols], R.DDPM_T, B, 4,
                  per // 4, int(clip), x.ptr)

    assert int(k["t"][0]) == 2
    outs = []
    for _ in range(2):
        x, e, z = Buf(B * per, k["x"]), Buf(B * per, k["e"]), Buf(B * per, k["z"])
        call(k["t"].to(F32), x, e, z)
        outs.append([x.take(B, per)])
        close("ds_ddpm_update clip=%d" % clip, outs[-1][0], k["ref"][0], k["ref"][1], R.TOL)
    same(*outs)
    for bad in (-1.0, float(R.DDPM_T), float("nan")):
        t = k["t"].to(F32)
        t[1] = bad
        x, e, z = Buf(B * per, k["x"]), Buf(B * per, k["e"]), Buf(B * per, k["z"])
        with pytest.raises(MaaError, match="outside"):
            call(t, x, e, z)
        got = x.take(B, per)
        keep = torch.arange(B) != 1
        assert torch.equal(got[1], k["x"][1]) and torch.equal(got[keep], k["ref"][0][keep]), bad
