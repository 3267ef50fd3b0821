"""The keyed dropout rule without a GPU: its constants, the prefix and shift properties of the mask, its statistics, the torch
fallback of het_amd.layers.KeyedDropout against the numpy reference bit for bit, and the module's counter and seed.  Every test
here fails on a tree without the feature.

The statistical bounds are 5 sigma of the binomial of each count (sigma = sqrt(q (1 - q) / n)); with the seeds fixed the tests are
deterministic, and the shares measured when the rule was written lie within 2.0 sigma."""
import math

import numpy as np
import pytest
import torch

from tests import _keyed_dropout_ref as ref
from tests._keyed_dropout_ref import same_bits

N_STAT = 1 << 20
SEEDS = (0, 1, 12345, (1 << 63) + 5)
DRAWS = (0, 1, 7)


def test_rates_thresholds_and_scales():
    from het_amd.layers import keyed_dropout_params
    want = {0.0: 0, 2.0 ** -16: 1, 0.1: 6554, 1.0 / 3.0: 21845, 0.5: 32768, 0.9: 58982, 65535.0 / 65536.0: 65535}
    assert set(want) == set(ref.RATES)
    for p, T in want.items():
        t, scale = ref.params(p)
        assert t == T and scale.dtype == np.float32 and float(scale) == float(np.float32(65536.0 / (65536 - T))), p
        assert keyed_dropout_params(p) == (T, float(scale)), p  # the module's own constants
    assert ref.params(0.0) == (0, np.float32(1.0)) and bool(ref.mask(3, 0, 0, 4096, 0.0).all())  # p = 0 keeps everything at scale 1
    assert ref.params(0.5)[1] == np.float32(2.0)
    assert ref.params(1.0 - 1e-9) == (65535, np.float32(65536.0))  # (p * 65536 rounds to 65536: the largest rate that keeps something)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            keyed_dropout_params(bad)


def test_prefix_property():
    """A tail of n % 4 elements uses the low fields of its group: n = 10 is the first 10 of n = 12."""
    from het_amd.layers import keyed_dropout_mask
    assert np.array_equal(keyed_dropout_mask((1 << 63) + 5, 3, 0, 10, 1.0 / 3.0).numpy(), ref.mask((1 << 63) + 5, 3, 0, 12, 1.0 / 3.0)[:10])
    for p in (0.1, 0.5, 0.9):
        assert np.array_equal(ref.mask(12345, 3, 0, 10, p), ref.mask(12345, 3, 0, 12, p)[:10])
        assert np.array_equal(ref.mask(12345, 3, 8, 5, p), ref.mask(12345, 3, 8, 4096, p)[:5])


@pytest.mark.parametrize("shift", [4, 4 * 257, 1 << 40])
def test_shift_property(shift):
    """mask(base = 4k, n) is mask(0, n + 4k)[4k:]; for 4k = 2^40 the long mask is not built: the fields are compared group by group
    against keys taken at the group indices themselves (above 2^32)."""
    from het_amd.sampling import keyed_keys
    n = 1001
    got = ref.mask(7, 2, shift, n, 0.5)
    if shift < (1 << 30):
        assert np.array_equal(got, ref.mask(7, 2, 0, n + shift, 0.5)[shift:])
    i = np.uint64(shift) + np.arange(n, dtype=np.uint64)
    key = keyed_keys(7, 2, i // np.uint64(4))
    assert int((i // np.uint64(4)).max()) >= (1 << 32) or shift < (1 << 40)
    field = (key >> (np.uint64(16) * (i % np.uint64(4)))) & np.uint64(0xFFFF)
    assert np.array_equal(got, field >= np.uint64(32768))
    from het_amd.layers import keyed_dropout_mask  # the int64 emulation of the fallback gives the uint64 bits
    assert np.array_equal(keyed_dropout_mask(7, 2, shift, n, 0.5).numpy(), got)


def test_dropped_share():
    worst = 0.0
    for seed in SEEDS:
        for draw in DRAWS:
            for p in (0.1, 0.5, 0.9, 1.0 / 3.0):
                q = ref.params(p)[0] / 65536.0
                share = 1.0 - float(ref.mask(seed, draw, 0, N_STAT, p).mean())
                sigma = math.sqrt(q * (1 - q) / N_STAT)
                worst = max(worst, abs(share - q) / sigma)
                assert abs(share - q) <= 5 * sigma, (seed, draw, p, share, q)
    print(f"dropped share: at most {worst:.2f} sigma from T / 65536")


def test_draws_are_independent():
    from het_amd.layers import keyed_dropout_mask
    a, b = ref.mask(12345, 0, 0, N_STAT, 0.5), ref.mask(12345, 1, 0, N_STAT, 0.5)
    assert np.array_equal(keyed_dropout_mask(12345, 1, 0, N_STAT, 0.5).numpy(), b)  # (the torch emulation, at this size too)
    agree = float((a == b).mean())
    print(f"masks of draw 0 and draw 1 agree on {agree:.5f}")
    assert abs(agree - 0.5) <= 5 * math.sqrt(0.25 / N_STAT)


def test_fields_of_a_group_are_independent():
    m = ref.mask(12345, 0, 0, N_STAT, 0.5).reshape(-1, 4)
    sigma = math.sqrt(0.25 / m.shape[0])
    for a in range(4):
        for b in range(a + 1, 4):
            agree = float((m[:, a] == m[:, b]).mean())
            assert abs(agree - 0.5) <= 5 * sigma, (a, b, agree)


def test_column_rates_of_a_64_wide_view():
    m = ref.mask(12345, 0, 0, N_STAT, 0.5).reshape(-1, 64)
    rates = m.mean(axis=0)
    print(f"per-column keep rates {rates.min():.4f} .. {rates.max():.4f}")
    assert np.abs(rates - 0.5).max() <= 5 * math.sqrt(0.25 / m.shape[0])


def test_specials_land_on_kept_and_dropped_positions():
    y = ref.special_input(4097, torch.float32, 1)
    kept = torch.from_numpy(ref.mask(12345, 0, 0, 4097, 0.5))
    for s in ref.SPECIALS:
        at = torch.isnan(y) if math.isnan(s) else (y == s) & (torch.signbit(y) == (math.copysign(1.0, s) < 0))
        assert bool((at & kept).any()) and bool((at & ~kept).any()), s


@pytest.mark.parametrize("relu", [False, True], ids=["none", "relu"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5, 65535.0 / 65536.0])
def test_module_on_cpu_is_the_reference_bit_for_bit(p, dtype, relu):
    from het_amd.layers import KeyedDropout
    n = 4097
    y = ref.special_input(n, dtype, 1).requires_grad_(True)
    go = ref.special_input(n, dtype, 2)
    m = KeyedDropout(p, "relu" if relu else None, seed=12345)
    out = m(y, draw=3)
    assert out.dtype == dtype and m.draw == 0
    want = ref.forward(y, p, 12345, 3, relu)
    same_bits(out, want, "out")
    if p == 0.5:
        dropped = torch.from_numpy(~ref.mask(12345, 3, 0, n, p))
        assert bool((out.detach()[dropped] == 0).all()) and not bool(torch.signbit(out.detach()[dropped]).any())  # +0, NaN and inf too
    out.backward(go)
    same_bits(y.grad, ref.backward(go, want, p, 12345, 3, relu), "grad_y")
    # a strided view takes the same composition: the mask follows the logical (contiguous) order
    y2 = ref.special_input(2 * n, dtype, 1)[::2]
    same_bits(m(y2, draw=3), ref.forward(y2.contiguous(), p, 12345, 3, relu), "strided input")
    # another dtype: computed in fp32, cast back
    y64 = ref.special_input(n, torch.float32, 1)
    same_bits(m(y64.double(), draw=3).float(), ref.forward(y64, p, 12345, 3, relu), "float64 input")


def test_counter_and_draw_override():
    from het_amd.layers import KeyedDropout
    m = KeyedDropout(0.5, "relu", seed=9)
    y = torch.randn(37)
    a, b = m(y), m(y)
    assert m.draw == 2
    same_bits(a, ref.forward(y, 0.5, 9, 0, True), "first call")
    same_bits(b, ref.forward(y, 0.5, 9, 1, True), "second call")
    same_bits(m(y, draw=0), a, "draw=0")
    assert m.draw == 2  # (draw= leaves the counter alone)
    m.eval()
    assert torch.equal(m(y), torch.relu(y)) and m.draw == 2
    m.train()
    z = KeyedDropout(0.0, None, seed=9)
    assert z(y) is y and z.draw == 0  # nothing to drop: the activation alone, the counter does not move
    with pytest.raises(ValueError):
        KeyedDropout(0.5, "gelu")
    with pytest.raises(ValueError):
        KeyedDropout(1.0)


def test_each_call_keeps_its_own_draw():
    """Two calls of one module, both outputs alive, then one backward: each input's gradient carries the mask of its own draw."""
    from het_amd.layers import KeyedDropout
    m = KeyedDropout(0.5, None, seed=5)
    y0, y1 = torch.randn(101, requires_grad=True), torch.randn(101, requires_grad=True)
    o0, o1 = m(y0), m(y1)
    go = torch.randn(101)
    (o0 * go).sum().add((o1 * go).sum()).backward()
    same_bits(y0.grad, ref.backward(go, None, 0.5, 5, 0), "draw 0")
    same_bits(y1.grad, ref.backward(go, None, 0.5, 5, 1), "draw 1")
    assert not torch.equal(y0.grad, y1.grad)


def test_seed_from_the_default_generator():
    from het_amd.layers import KeyedDropout
    torch.manual_seed(77)
    a, b = KeyedDropout(), KeyedDropout()
    torch.manual_seed(77)
    c = KeyedDropout()
    assert a.seed == c.seed and a.seed != b.seed and (a.p, a.activation, a.draw) == (0.5, None, 0)
    torch.manual_seed(77)
    before = torch.rand(3)
    torch.manual_seed(77)
    KeyedDropout(seed=4)  # a given seed consumes nothing
    assert torch.equal(torch.rand(3), before)
