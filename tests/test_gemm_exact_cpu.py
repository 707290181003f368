"""The element-wise GEMM check itself, tested without a GPU (tests/gemm_exact_helpers.py keeps test_gemm_exact_gpu.py honest):
(a) a k-ordered float32 fmaf chain, whole or cut into split-K partial sums, stays within Q / 2 of float64 on every element;
(b) every planted kernel fault fails the check at the planted elements, even with the bar at its cap of 64 * 2^-24;
(c) the exact-zero / untouched / "either" row regions and the 25 % exclusion cap behave as stated."""
import math

import pytest
import torch

from tests import gemm_exact_helpers as gx

MODES = ['bf16', 'fp16', 'f32']


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return scale * torch.randn(*shape, generator=g)


def rounded(t, mode):
    return t if mode == 'f32' else t.to(gx.H16[mode]).float()


def fmaf_chain(a, b, parts=1):
    """sum_k a[:, k] b[:, k] as the MFMA forms it: one float32 accumulator per element, products added in k order with a single
    rounding each (the float64 sum of a float32 accumulator and a float32 x float32 product is exact to well below half a float32
    step, so rounding it to float32 IS the fused multiply-add).  ``parts`` > 1: the K range cut into that many chains, the partial
    sums added afterwards in float32 (split-K)."""
    M, K = a.shape
    a64, b64 = a.double(), b.double()
    total = torch.zeros(M, dtype=torch.float32)
    edges = [round(i * K / parts) for i in range(parts + 1)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        acc = torch.zeros(M, dtype=torch.float32)
        for k in range(lo, hi):
            acc = (acc.double() + a64[:, k] * b64[:, k]).float()
        total = acc if parts == 1 else (total.double() + acc.double()).float()
    return total


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('K', [192, 384, 3072])
def test_fmaf_chain_stays_within_half_q(mode, K):
    M = 300
    x = rounded(randn(M, K, seed=K), mode)
    w = rounded(randn(M, K, seed=K + 1, scale=1 / math.sqrt(K)), mode)
    y64 = (x.double() * w.double()).sum(1)
    S = (x.double().abs() * w.double().abs()).sum(1)
    for parts in (1, 2, 4, 16):
        err = (fmaf_chain(x, w, parts).double() - y64).abs()
        worst = float((err / S).max()) / gx.U24
        print(f'{mode} K={K} parts={parts}: max |err| / S = {worst:.2f} x 2^-24')
        assert bool((err <= gx.Q0 / 2 * S).all()), (parts, worst)


@pytest.mark.parametrize('mode', MODES)
def test_weight_gradient_chain_over_9000_tokens_stays_within_half_q(mode):
    M, T = 256, 9000
    dy, x = rounded(randn(M, T, seed=5), mode), rounded(randn(M, T, seed=6), mode)
    y64 = (dy.double() * x.double()).sum(1)
    S = (dy.double().abs() * x.double().abs()).sum(1)
    for parts in (1, 2, 4, 16):
        err = (fmaf_chain(dy, x, parts).double() - y64).abs()
        worst = float((err / S).max()) / gx.U24
        print(f'{mode} wgrad T={T} parts={parts}: max |err| / S = {worst:.2f} x 2^-24')
        assert bool((err <= gx.Q0 / 2 * S).all()), (parts, worst)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def case():
    """One deep convolution (K = 3 x 1024 = 3072) on bf16-rounded operands: float64 reference, magnitude sums, nothing modified later."""
    B, N, Cin, Cout = 2, 130, 1024, 16
    x = gx.operand64(randn(B, N, Cin, seed=1), 'bf16')
    w = gx.operand64(randn(Cout, Cin, 3, seed=2, scale=1 / math.sqrt(3 * Cin)), 'bf16')
    bias = randn(Cout, seed=3, scale=0.1).double()
    acc, S0 = gx.conv64(x, w)                       # without the bias
    y, S = gx.conv64(x, w, bias)
    return dict(x=x, w=w, bias=bias, acc=acc, y=y, S=S, B=B, N=N, Cin=Cin, Cout=Cout)


def failing_share(v, planted):
    assert not bool((v.fail & ~planted).any()), 'an element nobody touched fails'
    return float(v.fail[planted].float().mean())


def test_unplanted_result_passes(case):
    v = gx.check(case['y'].float(), case['y'], case['S'], q=gx.Q0)
    assert v.ok and v.ratio < 1.0                    # a float32 rounding of the exact value: far inside


def test_one_product_dropped_at_the_k_tail(case):
    c = case
    dev = c['y'].clone()
    rows = [0, 63, 64, 128]
    for n in rows:                                   # the last input channel of the n + 1 tap: the last product of the K loop
        dev[1, n] -= c['x'][1, n + 1, c['Cin'] - 1] * c['w'][:, c['Cin'] - 1, 2]
    planted = torch.zeros_like(dev, dtype=torch.bool)
    planted[1, rows] = True
    signal = ((dev - c['y']).abs() / c['S'])[planted]
    print(f'median signal {float(signal.median()):.2e} S = {float(signal.median()) / gx.Q0:.0f} Q')
    assert failing_share(gx.check(dev, c['y'], c['S'], q=gx.Q_CAP), planted) >= 0.5


def test_one_eight_element_slot_dropped(case):
    c = case
    dev = c['y'].clone()
    dev[0, 64:80] -= c['x'][0, 64:80, 512:520] @ c['w'][:, 512:520, 1].T          # one 16-token MFMA column tile loses the slot
    planted = torch.zeros_like(dev, dtype=torch.bool)
    planted[0, 64:80] = True
    # the lost sum of 8 products is a random number of sigma = sqrt(8) / 55 = 0.05 against a bar of 64 * 2^-24 * S = 1.3e-4: it hides
    # below the bar with probability ~2e-3 per element (where the eight products happen to cancel, nothing is wrong to any check)
    assert failing_share(gx.check(dev, c['y'], c['S'], q=gx.Q_CAP), planted) >= 0.98


def test_bias_omitted_on_one_channel(case):
    c = case
    ch = int(c['bias'].abs().argmax())
    dev = c['y'].clone()
    dev[:, :, ch] -= c['bias'][ch]
    planted = torch.zeros_like(dev, dtype=torch.bool)
    planted[:, :, ch] = True
    assert failing_share(gx.check(dev, c['y'], c['S'], q=gx.Q_CAP), planted) == 1.0


def test_previous_row_tap_missing_on_the_first_row_of_a_tile(case):
    c = case
    dev = c['y'].clone()
    planted = torch.zeros_like(dev, dtype=torch.bool)
    for n in (64, 128):
        dev[:, n] -= c['x'][:, n - 1] @ c['w'][:, :, 0].T
        planted[:, n] = True
    assert failing_share(gx.check(dev, c['y'], c['S'], q=gx.Q_CAP), planted) == 1.0


def test_one_row_beyond_len_not_zeroed_under_mask_rows(case):
    c = case
    lens = torch.tensor([130, 65])
    valid = gx._row_mask(c['N'], lens, 'cpu')
    y = c['y'] * valid
    dev = y.clone()
    assert gx.check(dev, y, c['S'], q=gx.Q_CAP, exact=~valid).ok
    dev[1, 65] = c['y'][1, 65]                       # the row at len keeps its convolution
    planted = torch.zeros_like(dev, dtype=torch.bool)
    planted[1, 65] = True
    assert failing_share(gx.check(dev, y, c['S'], q=gx.Q_CAP, exact=~valid), planted) == 1.0


def test_out_scale_not_applied_to_the_bias(case):
    c = case
    y, g = gx.epilogue64(c['y'], c['S'], out_scale=-0.5)
    dev = -0.5 * c['acc'] + c['bias']
    v = gx.check(dev, y, c['S'], g, q=gx.Q_CAP)
    assert bool(v.fail.all())
    assert gx.check(-0.5 * (c['acc'] + c['bias']), y, c['S'], g, q=gx.Q0).ok


def test_sixteen_bit_output_rounded_twice(case):
    c = case
    y32 = c['y'].float()
    once = y32.to(torch.bfloat16)
    assert gx.check(once, c['y'], c['S'], q=gx.Q0, out16='bf16').ok
    chopped = (y32.view(torch.int32) & ~0x1FFF).view(torch.float32)        # truncated to 10 mantissa bits, then rounded to 8
    twice = chopped.to(torch.bfloat16)
    v = gx.check(twice, c['y'], c['S'], q=gx.Q_CAP, out16='bf16')
    differs = twice != once
    assert not v.ok and not bool((v.fail & ~differs).any())
    print(f'{int(v.fail.sum())} of {int(differs.sum())} misrounded elements leave the bound')


def test_fp16_output_gets_half_a_subnormal_step():
    y = torch.tensor([[[3.0e-8, 1.0, -2.9e-8]]], dtype=torch.float64)
    S = torch.full_like(y, 1e-9)
    assert gx.check(y.float().to(torch.float16), y, S, out16='fp16').ok    # 3e-8 rounds to 0 or 2^-24: inside 2^-25
    bad = y.float().to(torch.float16).clone()
    bad[0, 0, 0] = 2.0 ** -23
    assert not gx.check(bad, y, S, out16='fp16').ok


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
def test_row_regions_and_exact_conditions():
    B, N, C = 3, 300, 8
    lens = torch.tensor([300, 129, 127])
    y = randn(B, N, C, seed=9).double()
    S = y.abs() + 1.0
    must, beyond, between = gx.row_regions(N, lens, 1, 'cpu')
    assert int(must[1].sum()) == 130 and int(between[1].sum()) == 126 and int(beyond[1].sum()) == 44
    assert int(must[2].sum()) == 128 and int(between[2].sum()) == 0 and int(beyond[2].sum()) == 172       # len + halo on the tile edge
    assert int(must[0].sum()) == 300                                                                       # len + halo clipped to N
    # non-accumulating: zeros beyond, either in between
    dev = (y * (must | between)).float()
    assert gx.check(dev, y, S, must=must, exact=beyond, between=between).ok
    dev0 = (y * must).float()
    assert gx.check(dev0, y, S, must=must, exact=beyond, between=between).ok
    mixed = dev0.clone()
    mixed[1, 130:200] = y[1, 130:200].float()                     # a 64-token kernel computes part of the open rows
    assert gx.check(mixed, y, S, must=must, exact=beyond, between=between).ok
    bad = dev0.clone()
    bad[1, 140, 3] = 0.5 * y[1, 140, 3].float()                   # neither zero nor the convolution
    bad[1, 290, 0] = 1e-30                                        # a skipped tile that is not exactly zero
    bad[0, 5, 1] += 1e-3                                          # and an ordinary wrong element
    v = gx.check(bad, y, S, must=must, exact=beyond, between=between)
    assert sorted(tuple(int(i) for i in r) for r in v.fail.nonzero()) == [(0, 5, 1), (1, 140, 3), (1, 290, 0)]
    assert '(1, 140, 3)' in v.describe()
    # accumulating: untouched beyond, bit for bit
    base = randn(B, N, C, seed=10)
    base[2, 200, 0] = -0.0
    full = base.double() + y
    acc = torch.where((must | between).expand_as(base), full.float(), base)
    Sa = S + base.double().abs()
    assert gx.check(acc, full, Sa, must=must, exact=beyond, exact_value=base, between=between).ok
    flipped = acc.clone()
    flipped[2, 200, 0] = 0.0                                      # equal in value, not in bits
    v = gx.check(flipped, full, Sa, must=must, exact=beyond, exact_value=base, between=between)
    assert [tuple(int(i) for i in r) for r in v.fail.nonzero()] == [(2, 200, 0)]
    # a NaN never passes
    nan = dev.clone()
    nan[0, 0, 0] = float('nan')
    assert not gx.check(nan, y, S, must=must, exact=beyond, between=between).ok


def test_exclusion_cap_and_region_cover():
    B, N, C = 2, 130, 4
    y = randn(B, N, C, seed=11).double()
    S = y.abs() + 1.0
    must, beyond, between = gx.row_regions(N, torch.tensor([130, 1]), 0, 'cpu')       # 127 of 260 rows are open
    with pytest.raises(AssertionError, match='excluded'):
        gx.check(y.float(), y, S, must=must, exact=beyond, between=between)
    with pytest.raises(AssertionError, match='cover'):
        gx.check(y.float(), y, S, must=must, exact=beyond)                            # the open rows belong to no region
    with pytest.raises(AssertionError, match='cap'):
        gx.check(y.float(), y, S, q=2 * gx.Q_CAP)
    for tile in (64, 128):
        for Bn, Nn in ((2, 130), (3, 150), (13, 640), (4, 300), (64, 200), (5, 1)):
            for rot in range(4):
                for halo in (0, 1):
                    lens = gx.pick_lens(Bn, Nn, tile, rot, open_halo=halo)
                    _, _, btw = gx.row_regions(Nn, torch.tensor(lens), halo, 'cpu', tile=tile)
                    assert float(btw.float().mean()) < gx.MAX_EXCLUDED, (Bn, Nn, tile, rot, halo, lens)
    assert set(gx.pick_lens(13, 640, 128)) == {640, 129, 127, 1, 128}
    assert gx.pick_lens(5, 1, 64) == [1] * 5


def test_launch_plan_predicates():
    """the shapes of test_gemm_exact_gpu.py land on the paths their table claims: asked of the library's own dispatch rule"""
    conv = lambda *a, **k: gx.path(gx.conv_plan(*a, **k))
    wgrad = lambda mode, Cin, Cout: gx.path(gx.wgrad_plan(mode, 2, 130, Cin, Cout, 1))
    chunk = lambda taps, dy16, x16: gx.wgrad_plan('bf16', 2, 130, 128, 136, taps, dy16, x16).chunk
    assert conv('f32', 3, 129, 80, 136, 3) == 'f32_64' and conv('f32', 5, 1, 192, 128, 1) == 'f32_64'
    assert conv('f32', 64, 200, 64, 1024, 3) == 'f32_128' and conv('f32', 64, 200, 64, 1024, 1) == 'f32_128'
    assert conv('bf16', 4, 37, 192, 384, 1) == 'h16_64' and conv('fp16', 3, 150, 128, 384, 1) == 'h16_64'
    for shape in ((3, 150, 128, 1024, 3), (2, 130, 80, 136, 3), (4, 130, 288, 128, 3), (64, 200, 192, 1024, 1)):
        assert conv('bf16', *shape) == 'h16_128', shape
    assert gx.conv_plan('bf16', 1, 1, 288, 128, 1).cinp == 320
    assert conv('bf16', 13, 640, 80, 136, 3) == 'ws' and conv('bf16', 13, 640, 128, 384, 1) == 'ws'
    assert conv('bf16', 12, 640, 128, 384, 1) == 'h16_64'                      # 60 token tiles: below the threshold
    assert conv('bf16', 4, 300, 256, 128, 3) == 'dk' and conv('bf16', 4, 300, 320, 80, 1) == 'dk'
    assert conv('bf16', 1100, 130, 256, 128, 3) == 'dk' and conv('bf16', 1100, 130, 128, 256, 1) == 'ws'
    assert gx.plain_tile_order(1100) and not gx.plain_tile_order(1024)
    assert wgrad('f32', 80, 136) == 'f32' and wgrad('bf16', 192, 4) == 'f32'
    assert wgrad('bf16', 128, 384) == 'narrow' and wgrad('bf16', 256, 136) == 'narrow'
    assert wgrad('fp16', 1024, 512) == 'wide'
    assert chunk(3, True, False) == 64 and chunk(3, True, True) == 128 and chunk(1, False, False) == 128
    assert gx.ff_pair_plan(4, 127).tok == 62 and gx.ff_pair_plan(32, 379).tok == 126 and gx.ff_pair_plan(23, 379).tok == 62
