"""CPU checks of the attention test helpers (tests/attn_ref.py), and the statement that the gates of
tests/test_gpu_attention.py can be met: a float64 emulation of the fused kernel's design -- bf16 or bf16 hi + lo operands,
fp32 scores, rounded softmax weights -- stays within HALF of each gate on the inputs the GPU tests use."""
import math

import pytest
import torch

from tests import attn_ref as R


def test_attention_ref_against_loops():
    B, heads, dh, Nq, Nk = 2, 3, 8, 5, 5
    q, k, v = R.random_qkv(B, heads, dh, Nq, Nk, seed=1, distinct_heads=True)
    alpha = 0.3
    for causal in (False, True):
        ref = R.attention_ref(q, k, v, heads, alpha, causal)
        for b in range(B):
            for h in range(heads):
                for i in range(Nq):
                    keys = range(i + 1) if causal else range(Nk)
                    w = [math.exp(alpha * sum(float(q[b, i, h, d]) * float(k[b, j, h, d]) for d in range(dh))) for j in keys]
                    for d in range(dh):
                        o = sum(wj * float(v[b, j, h, d]) for wj, j in zip(w, keys)) / sum(w)
                        assert abs(o - float(ref[b, i, h, d])) < 1e-12


def test_split32_line_format():
    """[32 bf16 hi | 32 bf16 lo] per 32 columns, pitch unchanged: decode a buffer built here bit by bit, then the encoder."""
    rows, C, ld = 3, 64, 80
    hi = torch.arange(rows * C, dtype=torch.float32).reshape(rows, C) % 97 + 1.0       # exact in bf16
    lo = torch.full((rows, C), 2.0 ** -10) * (1 + torch.arange(C) % 3)                   # exact in bf16, below half an ulp of hi
    raw = torch.zeros(rows, 2 * ld, dtype=torch.bfloat16)
    for r in range(rows):
        for c in range(C):
            raw[r, (c // 32) * 64 + c % 32] = hi[r, c]
            raw[r, (c // 32) * 64 + 32 + c % 32] = lo[r, c]
    raw[:, 2 * C:] = float("nan")                                                        # pitch padding is never decoded
    buf = raw.view(torch.float32)
    assert buf.shape == (rows, ld)
    assert torch.equal(R.split32_decode(buf, rows, C), (hi + lo).to(torch.float64))
    assert torch.equal(R.split32_encode(hi + lo, ld)[:, :C], buf[:, :C])
    x = torch.randn(7, 96, generator=R.gen(2)) * 100
    dec = R.split32_decode(R.split32_encode(x), 7, 96)
    assert bool(((dec - x.to(torch.float64)).abs() <= 2.0 ** -16 * x.abs().to(torch.float64)).all())
    assert not torch.equal(dec, x.to(torch.float64))                                     # ... and it is a rounding, not a copy


def _emulated_within_half_gate(name, q, k, v, alpha, ref, causal=False):
    for precision, terms in R.TERMS.items():
        e = R.rel_max(R.attention_emulated(q, k, v, alpha, terms, causal), ref)
        assert e <= 0.5 * R.GATE[precision], (name, precision, e)


@pytest.mark.parametrize("dh", R.FLASH_DH + (48,))
def test_one_hot_inputs_have_their_margin_and_the_design_meets_the_gates(dh):
    alpha = dh ** -0.5
    for Nq, Nk in R.ONE_HOT_SHAPES:
        for name in R.ONE_HOT_MAPS:
            q, k, v, j = R.one_hot_qkv(1, 1, dh, Nq, Nk, alpha, name, seed=600 + dh)
            ref, scores = R.attention_ref(q, k, v, 1, alpha, return_scores=True)
            assert float(scores.max()) > R.ONE_HOT_NATS - 1e-3
            assert R.one_hot_margin(scores, j) >= R.ONE_HOT_MIN_MARGIN
            exact = v[:, j]
            assert R.rel_max(ref, exact) < 1e-12
            _emulated_within_half_gate((dh, Nq, Nk, name), q, k, v, alpha, exact)
    if dh == 32:       # the three maps reach every key-slot of a 32-key tile, in both halves of the wave
        assert set((R.one_hot_map("scatter", 780, 780) % 32).tolist()) == set(range(32))


@pytest.mark.parametrize("dh", R.FLASH_DH)
def test_sharp_inputs_the_design_meets_the_gates(dh):
    alpha = dh ** -0.5
    cases = [s + (False,) for s in R.SHARP_SHAPES] + [(R.SHARP_CAUSAL_L, R.SHARP_CAUSAL_L, True)]
    for Nq, Nk, causal in cases:
        for scale in R.SHARP_SCALES:
            q, k, v = R.random_qkv(1, 1, dh, Nq, Nk, seed=34, qscale=scale)
            ref, scores = R.attention_ref(q, k, v, 1, alpha, causal, return_scores=True)
            if scale == 4.0 and Nk >= 780:
                assert float(scores[torch.isfinite(scores)].abs().max()) > 15.0      # the softmax is sharp indeed
            _emulated_within_half_gate((dh, Nq, Nk, scale), q, k, v, alpha, ref, causal)


@pytest.mark.parametrize("kind", R.CAUSAL_KINDS)
def test_causal_inputs_show_the_edge_and_the_design_meets_the_gates(kind):
    """One key too many (query i sees key i + 1) or too few (query i > 0 does not see key i) must be far outside the loosest
    gate; for the `random` kind that holds for the dropped key everywhere and for the extra key only at the smallest L."""
    for dh in (64, 80, 48):
        alpha = dh ** -0.5
        for L in (1, 2, 31, 32, 33, 64, 77, 128, 129, 200):
            q, k, v = R.causal_qkv(2, 1, dh, L, alpha, kind, seed=500 + dh)
            ref, s = R.attention_ref(q, k, v, 1, alpha, True, return_scores=True)
            _emulated_within_half_gate((kind, dh, L), q, k, v, alpha, ref, True)
            if L == 1:
                continue
            s = torch.matmul(q.double().permute(0, 2, 1, 3), k.double().permute(0, 2, 3, 1)) * alpha
            i = torch.arange(L)
            admit = i[None, :] > i[:, None] + 1
            drop = (i[None, :] >= i[:, None]) & (i[:, None] > 0)
            for name, mask in (("admit", admit), ("drop", drop)):
                wrong = torch.matmul(torch.softmax(s.masked_fill(mask, -math.inf), -1), v.double().permute(0, 2, 1, 3))
                e = R.rel_max(wrong.permute(0, 2, 1, 3), ref)
                if kind == "next" or name == "drop" or L == 2:
                    assert e > 4 * R.GATE["bf16"], (kind, dh, L, name, e)
