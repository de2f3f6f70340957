"""The per-element bounds of tests/test_gpu_vit.py speak for the kernels only if the arithmetic they describe stays inside them: a numpy fp32
emulation of the written contract of csrc/mpx_attn.h (three products per 32-wide MFMA step into an fp32 accumulator, 0.125 exact, the maximum
over the real keys, expf, the four partial sums of the weights in their fixed order, the weights split at 1024 x, P V in 32-key steps, ONE
division behind the whole sum, the re-split; for the token assembly one fp32 add and the re-split), run on the very draws the GPU tests use
(tests/attn_draws.py), against fp64.  The same run measures r_ref -- the emulation's worst err / B in units of 2^-22 -- and holds the recorded
table to the rule C_f = 4 r_ref rounded up to a power of two, and a fresh measurement within a factor of two of the record.  No GPU.
Measured here, printed on every run: see DESIGN.md 23."""
import math

import numpy as np
import pytest

import attn_draws as draws


def _report(key, got, want, mag):
    # the coefficient the magnitude term needs: what the absolute term 2^-24 (the floor of a split-fp16 pair, whose lo half is an fp16
    # subnormal under 2^-3 and whose hi half flushes under 2^-25) does not already cover
    r_ref = (np.maximum(np.abs(got.astype(np.float64) - want) - 2.0 ** -24, 0.0) / mag).max() / 2.0 ** -22
    rec, c_f = draws.R_REF[key], draws.C_F[key]
    worst = (np.abs(got.astype(np.float64) - want) / draws.tol(mag, c_f)).max()
    print("%s: r_ref %.4f x 2^-22 (recorded %.4f) -> C_f %g (recorded %g), emulation worst err / bound %.3f" % (key, r_ref, rec, draws.pow2_ceil(4 * r_ref), c_f, worst))
    assert c_f == draws.pow2_ceil(4 * rec) and 0.5 * rec <= r_ref <= 2.0 * rec, (key, r_ref, rec, c_f)
    assert worst <= 1.0, (key, worst)


@pytest.mark.parametrize("t,heads,b", draws.ATTN_CASES)
def test_attention_contract_stays_inside_its_bound(t, heads, b):
    x = draws.qkv_planes(b, t, heads, seed=1000 * t + heads)
    want, mag = draws.attn_want(x, heads)
    got = draws.emulate_attention(x, heads)
    live = mag > 0                                              # (a channel whose V is an exact zero on every key that has weight: the output is 0)
    assert live.mean() > 0.85 and (got[~live] == 0).all()
    _report(("attn", t, heads), got[live], want[live], mag[live])


def test_attention_draws_are_what_they_claim():
    """Exact zeros, both signs, every value a valid (hi, lo) pair; the x 8 band makes rows near one-hot, the x 1 / 8 band rows near uniform; V
    carries a per-channel offset."""
    t, heads = 197, 2
    x = draws.qkv_planes(1, t, heads, seed=1000 * t + heads)
    assert np.array_equal(draws.valid_pairs(x), x) and (x == 0).any() and (x < 0).any() and (x > 0).any()
    q, k, v = (z.astype(np.float64) for z in draws.heads_of(x, heads))
    s = 0.125 * (q @ k.transpose(0, 1, 3, 2))
    e = np.exp(s - s.max(-1, keepdims=True))
    peak = (e / e.sum(-1, keepdims=True)).max(-1)[0, 0]
    print("softmax peak: x 8 rows %.3f .. %.3f, x 1/8 rows %.4f .. %.4f (uniform: %.4f), other rows %.3f .. %.3f"
          % (peak[0::5].min(), peak[0::5].max(), peak[1::5].min(), peak[1::5].max(), 1.0 / t, peak[2::5].min(), peak[2::5].max()))
    assert np.median(peak[0::5]) > 0.5 and peak[1::5].max() < 2.0 / t
    assert np.abs(v.mean((0, 2))).mean() > 0.2          # the channel offset: a mean over tokens that is no sampling noise (0.07)


@pytest.mark.parametrize("b,t,d", draws.TOK_CASES)
def test_token_assembly_contract_stays_inside_its_bound(b, t, d):
    x, cls, pos = draws.tok_draw(b, t, d, seed=100 * t + d)
    want, mag = draws.tok_want(x, cls, pos)
    got = draws.emulate_tokens(x, cls, pos)
    live = mag > 0
    assert live.any() and (np.abs(got[~live]) == 0).all()        # 0 + 0 stays an exact zero
    _report(("tok", b, t, d), got[live], want[live], mag[live])


def test_the_table_is_complete_and_powers_of_two():
    assert all(("attn", t, h) in draws.C_F for t, h, _b in draws.ATTN_CASES) and all(("tok",) + c in draws.C_F for c in draws.TOK_CASES)
    assert len({(t, h) for t, h, _b in draws.ATTN_CASES}) == len(draws.ATTN_CASES)
    assert all(math.log2(v) == int(math.log2(v)) for v in draws.C_F.values())
    assert {t for t, _h, _b in draws.ATTN_CASES} == {1, 15, 16, 17, 50, 197} and {h for _t, h, _b in draws.ATTN_CASES} == {1, 2, 12}
    assert {b for _t, _h, b in draws.ATTN_CASES} == {1, 3}
