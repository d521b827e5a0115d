"""tests/tts_rows_ref.py on the CPU, no library: for every input tests/test_gpu_tts_ops.py uses, torch's own fp32 evaluation of
each reference stays within HALF of the gate the GPU test applies to the kernels, every exact comparison (energy bins, masks,
positions) has its margin from a threshold, checked in float64, and the builders produce the edge values they claim."""
import math

import pytest
import torch

from tests import fs2_plain_ref as FP
from tests import norm_ref as N
from tests import tts_rows_ref as R

F32, F64 = torch.float32, torch.float64


def half(got, ref, tol, what):
    r = N.rel_max(got, ref)
    assert r <= tol / 2, "%s: torch fp32 is %.3e from float64, more than half of %.1e" % (what, r, tol)
    return r


# ---- squeeze

@pytest.mark.parametrize("C", R.SQ_C)
@pytest.mark.parametrize("T", R.SQ_T)
@pytest.mark.parametrize("B", R.SQ_B)
def test_squeeze_reference_is_a_masked_copy(C, T, B):
    for masked in (False, True):
        z, mask = R.squeeze_input(C, T, B, masked)
        ref, ms = R.squeeze_ref(z, mask)
        got, ms32 = R.squeeze_ref(z, mask, F32)
        Ts = T // 2
        assert ref.shape == (B * Ts, 2 * C) and torch.isfinite(ref).all()          # the NaN of the odd frame is not in it
        assert torch.equal(ref, got.double()) and torch.equal(ms, ms32.double())
        assert bool(torch.isnan(z[:, T - 1]).all()) == bool(T % 2)
        # the same by plain indexing
        for b in range(B):
            for t in range(Ts):
                m = 1.0 if mask is None else float(mask[b, 2 * t + 1])
                want = torch.cat([z[b, 2 * t], z[b, 2 * t + 1]]) if m else torch.zeros(2 * C)
                assert torch.equal(ref[b * Ts + t].float(), want) and float(ms[b * Ts + t]) == m
        if masked:
            lengths = R.squeeze_lengths(T, B)
            assert any(n % 2 for n in lengths)
            for b, n in enumerate(lengths):
                if n % 2 and n < T:          # the pair the mask cuts: its first frame is live, and large
                    assert float(mask[b, n - 1]) == 1 and float(mask[b, n]) == 0 and float(z[b, n - 1, 0]) < -0.99 * R.HUGE
                    assert not bool(ref[b * Ts + n // 2].any())
            assert B == 1 or float(z.nan_to_num().abs().max()) > 0.99 * R.HUGE


# ---- gate

@pytest.mark.parametrize("H", R.GATE_H)
@pytest.mark.parametrize("rows", R.GATE_ROWS)
def test_gate_fp32_within_half(H, rows):
    y = R.gate_input(H, rows)
    ref = R.gate_ref(y)
    half(R.gate_ref(y, F32), ref, R.TOL_ROW, "gate")
    assert float(y.max()) == 100.0 and float(y.min()) == -100.0
    assert float(y[:, H:].max()) == 100.0 and float(y[:, H:].min()) == -100.0 and float(y[:, :H].max()) == 100.0
    swapped = R.gate_ref(torch.cat([y[:, H:], y[:, :H]], dim=1))
    assert N.rel_max(swapped, ref) > 0.1          # the halves the other way round is no small change
    assert float(ref.abs().max()) > 0.9 and bool((ref == 0).any() or (ref.abs() < 1e-30).any())


# ---- WN residual

@pytest.mark.parametrize("H", R.WN_H)
@pytest.mark.parametrize("rows", R.WN_ROWS)
def test_wn_residual_fp32_within_half(H, rows):
    x, rs, mask = R.wn_input(H, rows)
    assert rows == 1 or (float(mask[2]) == 0 and float(x[2].max()) > 0.99 * R.HUGE)
    for dt in (F64, F32):
        x1, s1 = R.wn_step_ref(x, None, rs[0], mask, True, False, dt)
        x2, s2 = R.wn_step_ref(x1, s1, rs[1], mask, False, False, dt)
        x3, s3 = R.wn_step_ref(x2, s2, rs[2], mask, False, True, dt)
        _, s4 = R.wn_step_ref(x, None, rs[2], mask, True, True, dt)
        if dt is F64:
            ref = (x1, s1, x2, s2, s3, s4)
            assert torch.equal(x3, x2)
            # the three layers as wavenet.py's loop runs them
            h, out = x.double(), torch.zeros(rows, H, dtype=F64)
            for i in range(3):
                r = rs[i].double()
                if i < 2:
                    h, out = (h + r[:, :H]) * mask.double()[:, None], out + r[:, H:]
                else:
                    out = out + r
            assert torch.equal(s3, out * mask.double()[:, None]) and torch.equal(x2, h)
        else:
            for got, want in zip((x1, s1, x2, s2, s3, s4), ref):
                half(got, want, R.TOL_ROW, "wn_residual")
        assert bool((x1[mask == 0] == 0).all()) and bool((s3[mask == 0] == 0).all()) and bool((s4[mask == 0] == 0).all())


# ---- block tail

@pytest.mark.parametrize("C", R.BT_C)
@pytest.mark.parametrize("sigmoid_scale", (0, 1))
def test_block_tail_fp32_within_half(C, sigmoid_scale):
    x, eo, mask, winv, an_bias, an_einv, rowld = R.bt_input(C, sigmoid_scale)
    ref = R.bt_ref(x, eo, mask, winv, an_bias, an_einv, sigmoid_scale)
    got = R.bt_ref(x, eo, mask, winv, an_bias, an_einv, sigmoid_scale, F32)
    for name, g, r in zip(("h_cpl", "h_inv", "h_act"), got, ref):
        print("block tail C %d ss %d %s: fp32 %.3e of the gate" % (C, sigmoid_scale, name, half(g, r, R.TOL_ROW, name) / R.TOL_ROW))
        assert bool((r[mask == 0] == 0).all())
    print("block tail C %d ss %d rowld: fp32 %.3e of the gate" % (C, sigmoid_scale, half(got[3], ref[3], R.TOL_REDUCE, "rowld") / R.TOL_REDUCE))
    half(rowld + got[3], rowld.double() + ref[3], R.TOL_REDUCE, "rowld accumulated")
    assert sorted(set(mask.tolist())) == [0.0, 0.5, 1.0]          # 0.5: every `* x_mask` of the three flows shows
    logs = eo[:, C:]
    lo, hi = (-14.0, 8.0) if sigmoid_scale else (-3.0, 3.0)
    assert float(logs.min()) == lo and float(logs.max()) == hi
    if sigmoid_scale:          # the floor matters: without it the scale at -14 is another
        s = torch.sigmoid(torch.tensor(lo + 2, dtype=F64))
        assert abs(math.log(1e-6 + float(s)) - math.log(float(s))) > 0.1
    w = winv.double()
    assert float(torch.linalg.cond(w)) < 5 and float((w - w.T).abs().min() + torch.eye(4).double().min()) >= 0
    off = ~torch.eye(4, dtype=torch.bool)
    assert bool(((w - w.T).abs()[off] > 0.05).all())          # a transposed read is no small change
    assert float((an_einv - 1).abs().max()) > 0.5 and float(an_bias.abs().max()) > 0.5
    # the mix by plain indexing: channel a * C + 2j + k is group 2a + k at position j
    h_cpl, h_inv = ref[0], ref[1]
    for j in (0, C // 2 - 1):
        grp = torch.stack([h_cpl[:, a * C + 2 * j + k] for a in (0, 1) for k in (0, 1)], dim=1)          # [rows, 4]
        z = grp @ w.T * mask.double()[:, None]
        for a in (0, 1):
            for k in (0, 1):
                assert torch.allclose(h_inv[:, a * C + 2 * j + k], z[:, 2 * a + k], rtol=0, atol=1e-9 * float(h_cpl.abs().max()))


# ---- log-determinant sum

@pytest.mark.parametrize("Ts", R.LD_TS)
@pytest.mark.parametrize("B", R.LD_B)
def test_logdet_bound_covers_fp32_orders(Ts, B):
    rowld, mask = R.logdet_input(Ts, B)
    ref = R.logdet_ref(rowld, mask, R.LD_PER_LEN)
    bound = R.logdet_bound(rowld, mask, R.LD_PER_LEN)
    assert bool((bound > 0).all()) and bool((bound < 2e-6 * (rowld.double().abs().sum(1) + 3.7 * mask.sum(1))).all())
    # the kernel's own order in fp32 on the CPU: strided partial sums, then the tree
    a, n = torch.zeros(B, 256), torch.zeros(B, 256)
    for t0 in range(0, Ts, 256):
        w = min(256, Ts - t0)
        a[:, :w] += rowld[:, t0:t0 + w]
        n[:, :w] += mask[:, t0:t0 + w]
    o = 128
    while o:
        a[:, :o] += a[:, o:2 * o]
        n[:, :o] += n[:, o:2 * o]
        o //= 2
    got = a[:, 0] + torch.tensor(R.LD_PER_LEN) * n[:, 0]
    assert bool(((got.double() - ref).abs() <= bound).all())
    assert B == 1 or (float(mask[1].sum()) < Ts or Ts == 1) and not bool(rowld[mask == 0].any())


# ---- positions and embedding

@pytest.mark.parametrize("T", R.TP_T)
def test_token_positions_equal_a_loop(T):
    tok = R.positions_tokens(T)
    pos = FP.positions(tok.long())
    assert torch.equal(pos, R.positions_loop(tok))
    assert int(pos[2].max()) == 0 and int(pos[0, 0]) == 0 and int(pos.max()) <= T
    if T > 3:
        assert int(pos[0, 3]) == 1
    if T >= 257:
        assert not bool(tok[1, 64:128].any()) and int(pos[1, 128]) == 65 and int(pos[1, 255]) == 192
    if T == 600:
        assert not bool(tok[1, 256:512].any()) and int(pos[1, 512]) == 193 and int(pos[0, 599]) > 256
    tab = R.positions_table(T)
    x, _ = R.embed_ref(tok, torch.zeros(R.TP_VOCAB, 4), tab, 1.0, 0)
    assert torch.equal(x, pos.double().reshape(-1, 1).repeat(1, 4))
    assert T + 1 < 2 ** 24          # the positions are exact in fp32


@pytest.mark.parametrize("H", R.EMB_H)
@pytest.mark.parametrize("rel", (0, 1))
def test_embed_fp32_within_half(H, rel):
    tok, E, pe, scale = R.embed_input(H, rel)
    ref, live = R.embed_ref(tok, E, pe, scale, rel)
    got, live32 = R.embed_ref(tok, E, pe, scale, rel, F32)
    half(got, ref, R.TOL_ROW, "embed")
    assert torch.equal(live, live32.double()) and int(tok.min()) < 0 and int(tok.max()) >= R.EMB_VOCAB + 7
    assert int((tok == 0).sum()) == 3 and bool((ref[tok.reshape(-1) == 0] == 0).all())
    # on clamped ids, fs2_plain_ref's own fp32 restatement (held to the goldens)
    cl = tok.long().clamp(0, R.EMB_VOCAB - 1)
    cl[tok == 0] = 0
    mine = got.reshape(R.EMB_B, R.EMB_T, H)
    theirs = FP.embed(dict(hidden_size=H, rel_pos=rel), cl, E)
    keep = torch.ones(R.EMB_B, R.EMB_T, dtype=torch.bool)
    keep[0, 5:] = False          # the negative token reads row 0 but is live and counts; fs2_plain_ref would take it for padding
    assert torch.allclose(mine[keep], theirs[keep], rtol=0, atol=2e-6 * float(ref.abs().max()))
    assert abs(scale - math.sqrt(H)) < 1e-6 * scale


# ---- speakers

@pytest.mark.parametrize("H", R.SPK_H)
def test_add_speaker_fp32_within_half(H):
    x, spk, mask, m2p = R.add_speaker_input(H)
    assert sorted(set(mask.tolist())) == [0.0, 0.5, 1.0] and int(m2p.min()) == 0 and int(m2p.max()) > 1
    assert R.SPK_T % 4 != 0          # row / T changes inside a workgroup
    for live in (mask != 0, m2p > 0):
        ref = R.add_speaker_ref(x, spk, live)
        half(R.add_speaker_ref(x, spk, live, F32), ref, R.TOL_ROW, "add_speaker")
        assert bool((ref[~live] == 0).all()) and bool(live.any()) and bool((~live).any())
    half_masked = R.add_speaker_ref(x, spk, mask != 0)[1]
    assert torch.equal(half_masked, x[1].double() + spk[0].double())          # 0.5 is live and does not scale


@pytest.mark.parametrize("H", R.SPK_H)
@pytest.mark.parametrize("B", R.GATHER_B)
def test_gather_builder(H, B):
    tabs, ids = R.gather_input(H, B)
    assert int(ids.min()) < 0 and int(ids.max()) >= R.GATHER_ROWS and R.GATHER_ROWS >= max(R.GATHER_B)
    assert not torch.equal(tabs[0], tabs[1]) and not torch.equal(tabs[1], tabs[2])
    a, b, c = R.gather_ref(tabs, ids, 1, B), R.gather_ref(tabs, ids, 0, B), R.gather_ref(tabs, None, 0, B)
    assert a.shape == (3, B, H) and torch.equal(c[1], tabs[1][:B])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2, B - 1], tabs[2][R.GATHER_ROWS - 1]) and torch.equal(a[0, 0], tabs[0][0])


# ---- energy tail

def test_planted_energy_lands_in_its_bins():
    e, bins = R.energy_planted()
    assert e.shape == (R.EN_B * R.EN_T,) and torch.equal(R.energy_bin_ref(e), bins)
    ok = ~torch.isnan(e)
    assert torch.equal(FP.energy_bin(e[ok]), bins[ok])          # fs2_plain_ref's fp32 form, the device's clamp included
    assert int(torch.isnan(e).sum()) == 1 and int(bins[torch.isnan(e)]) == 0
    k = R.EN_K
    assert float(e[0]) * 64 == k and float(e[1]) > k / 64 > float(e[2]) and (float(e[1]) - float(e[2])) < 2e-7
    assert bins[:3].tolist() == [k, k, k - 1] and float(e[3]) * 64 == 255 and int(bins.max()) == 255 and float(e.nan_to_num().min()) < 0
    # 64 e is exact in fp32 (a power of two), so the fp32 floor is the float64 floor on every finite value
    fin = torch.isfinite(e)
    assert torch.equal((e[fin] * 64.0).double(), e[fin].double() * 64.0)


@pytest.mark.parametrize("C", R.EN_C)
def test_energy_head_fp32_within_half_and_clear_of_the_bin_edges(C):
    x, gamma, beta, w, bias = R.energy_head_input(C)
    ref = R.energy_head_ref(x, gamma, beta, w, bias)
    got = R.energy_head_ref(x, gamma, beta, w, bias, F32)
    r = half(got, ref, R.TOL_REDUCE, "energy head")
    q = ref * 64.0
    dist = float((q - torch.round(q)).abs().min())
    print("energy head C %d: fp32 %.3e of the gate, nearest bin edge %.3e, margin %.3e" % (C, r / R.TOL_REDUCE, dist, R.energy_margin(ref)))
    assert dist >= R.energy_margin(ref) and R.energy_clear(ref)
    assert torch.equal(R.energy_bin_ref(ref), R.energy_bin_ref(got))          # fp32 and fp64 agree on every bin
    assert len(set(R.energy_bin_ref(ref).tolist())) > 5


@pytest.mark.parametrize("H", R.EN_H)
def test_energy_rows_fp32_within_half(H):
    acc, table, spk, m2p = R.energy_rows_input(H)
    e, bins = R.energy_planted()
    assert int(m2p.min()) < 0 and bool((m2p == 0).any()) and R.EN_T % 4 != 0
    for b, s in ((bins, spk), (bins, None), (None, spk), (None, None)):
        ref = R.energy_tail_ref(acc, b, table, s, m2p)
        half(R.energy_tail_ref(acc, b, table, s, m2p, F32), ref, R.TOL_ROW, "energy tail")
        assert bool((ref[m2p <= 0] == 0).all())
    # fs2_plain_ref's fp32 restatement (held to the goldens) on the finite planted values
    three = lambda t: t.reshape(R.EN_B, R.EN_T, *t.shape[1:])      # noqa: E731
    fin = ~torch.isnan(e)
    b32, dec32 = FP.energy_tail(three(acc), None, three(m2p.long()), table, spk, three(e.nan_to_num()))
    assert torch.equal(b32.reshape(-1)[fin], bins[fin])
    mine = R.energy_tail_ref(acc, bins, table, spk, m2p, F32)
    assert torch.equal(dec32.reshape(-1, H)[fin], mine[fin])


@pytest.mark.parametrize("rows", R.TGT_ROWS)
def test_tgt_builder(rows):
    m = R.tgt_input(rows)
    assert rows == 1 or (int(m.min()) < 0 and bool((m == 0).any()) and int(m.max()) > 0)


# ---- the model lengths

def test_plain_encode_reference_is_the_goldens():
    """plain_encode_ref in fp32 on the golden's own weights and tokens: the golden's encoder_out, xs and durations."""
    cfg, sd, g = FP.load_case("fs2_plain_b2_t33")
    tok = torch.from_numpy(g["txt_tokens"])
    enc, xs, dur = R.plain_encode_ref(sd, cfg, tok, F32)
    assert N.rel_max(enc, torch.from_numpy(g["encoder_out"])) < 1e-5 and N.rel_max(xs, torch.from_numpy(g["xs"])) < 1e-5
    assert torch.equal(dur, torch.from_numpy(g["dur_choice"]))
    cfg1, sd1 = R.plain_cfg()
    for T in R.PLAIN_T:
        tok = R.plain_tokens(T, cfg1["vocab_size"])
        assert not bool(tok[0, 64:128].any()) and not bool(tok[1, T - T // 10:].any()) and bool(tok[0, T - 1] != 0)
        assert int((tok[1, :T - T // 10] == 0).sum()) > 3 and int(FP.positions(tok).max()) > 256 - 64 - 10


def test_glow_long_case():
    cfg, sd, z, mask, cond = R.glow_long_case()
    assert z.shape[2] == 601 and z.shape[2] // 2 > 256 and int(mask[1].sum()) == 411 and int(mask[0].sum()) == 601
    assert (cond is None) == (cfg["gin_channels"] == 0)
