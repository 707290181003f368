"""The pitch-chain checks themselves, tested without a GPU (tests/pitch_exact_helpers.py keeps test_pitch_exact_gpu.py honest):
(a) the float64 restatement with rounding switched off is the plain torch chain, forward and gradient;
(b) the integer network of every exact-tier case is exactly representable in both 16-bit types and exercises zeros and both signs;
(c) the noise-floor constants behind the rounded tier's bars are what a fresh measurement gives;
(d) every planted kernel error breaks its check by at least 4 x the bar, or changes a bit of the exact tier."""
import pytest
import torch
import torch.nn.functional as F

from tests import pitch_exact_helpers as px

MODES = ['bf16', 'fp16']


@pytest.fixture(scope='module')
def dense():
    return px.dense_layers()


@pytest.fixture(scope='module')
def refs(dense):
    """mode -> ({case: (inputs, float64 results)}, tau): the rounded tier's cases, computed once"""
    out = {}
    for m in MODES:
        cases = {}
        for name in px.ROUNDED_CASES:
            inputs = px.rounded_inputs(name)
            cases[name] = (inputs, px.rounded_reference(dense, *inputs, m))
        out[m] = (cases, px.mask_tau([r for _, r in cases.values()]))
    return out


def torch_chain(mel, layers, dtype):
    """the chain of test_fused_pitch_predictor_chain_matches_torch_and_the_layer_launches: plain torch on the folded weights"""
    x, pre = mel.to(dtype), []
    for l in layers[:3]:
        v = F.conv1d(x, l['w'].to(dtype), l['b'].to(dtype), padding=1)
        pre.append(v)
        x = v.relu() * l['scale'].to(dtype)[None, :, None] + l['shift'].to(dtype)[None, :, None]
    return F.conv1d(x, layers[3]['w'][:1].to(dtype), layers[3]['b'][:1].to(dtype), padding=1)[:, 0], pre


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
def test_chain64_without_rounding_is_the_plain_torch_chain(dense):
    mel, dpp, base, lens = px.rounded_inputs('lengths')
    pp, pre = px.chain64(mel, dense, None, lens)
    pp_t, pre_t = torch_chain(mel, dense, torch.float32)
    assert float((pp - pp_t.double()).abs().max()) <= 1e-5 * float(pp_t.abs().max())
    for a, b in zip(pre, pre_t):
        assert float((a - b.double()).abs().max()) <= 1e-5 * float(b.abs().max())


def test_chain64_bwd_at_its_own_signs_is_autograd(dense):
    mel, dpp, base, lens = px.rounded_inputs('lengths')
    pp, pre = px.chain64(mel, dense, None, lens)
    grad = px.chain64_bwd(dpp, px.signs64(pre), dense, None)
    m = mel.double().requires_grad_(True)
    pp_t, _ = torch_chain(m, dense, torch.float64)
    (pp_t * dpp.double()).sum().backward()
    assert float((pp - pp_t.detach()).abs().max()) <= 1e-12 * float(pp_t.detach().abs().max())
    assert float((grad - m.grad).abs().max()) <= 1e-12 * float(m.grad.abs().max())


def test_chain64_treats_frames_past_rows_exist_as_padding(dense):
    """a stored tensor with rows_exist equals the tensor cut to the existing frames, whatever sits beyond them (NaN included)"""
    mel, dpp, base, lens = px.rounded_inputs('lengths')
    mel, dpp = mel[:2, :, :140].clone(), dpp[:2, :140].clone()
    ex, ln = [100, 130], [1, 122]
    pp_c, pre_c = px.chain64(mel[1:, :, :130], dense, 'bf16', ln[1:])
    grad_c = px.chain64_bwd(dpp[1:, :130], px.signs64(pre_c), dense, 'bf16')
    mel[0, :, 100:], mel[1, :, 130:], dpp[0, 100:], dpp[1, 130:] = float('nan'), float('nan'), float('nan'), float('nan')
    pp, pre = px.chain64(mel, dense, 'bf16', ln, ex)
    sg = [s | ~px.exist_mask(2, 140, ex, 'cpu')[:, None, :] for s in px.signs64(pre)]        # any bits beyond the existing frames
    grad = px.chain64_bwd(dpp, sg, dense, 'bf16', ex)
    assert torch.equal(pp[1, :130], pp_c[0]) and torch.equal(grad[1, :, :130], grad_c[0])
    assert not grad[:, :, 130:].any() and not grad[0, :, 100:].any() and bool(torch.isfinite(pp).all())


def test_mask_words_round_trip():
    g = torch.Generator().manual_seed(3)
    signs = torch.rand(5, 7, 3, 256, generator=g) < 0.5
    words = px.encode_masks(signs)
    assert words.shape == (5, 7, 3, 8) and words.dtype == torch.int32 and bool((words < 0).any())
    assert torch.equal(px.decode_masks(words), signs)
    one = torch.zeros(1, 1, 3, 8, dtype=torch.int32)
    one[0, 0, 1, 2] = 1 << 5                              # bit 5 of word 2 of layer 1 is channel 69
    dec = px.decode_masks(one)
    assert int(dec.sum()) == 1 and bool(dec[0, 0, 1, 69])
    one[0, 0, 1, 2] = -2 ** 31                            # bit 31: channel 95
    dec = px.decode_masks(one)
    assert int(dec.sum()) == 1 and bool(dec[0, 0, 1, 95])
    assert [s.shape for s in px.signs_of(words)] == [(5, 256, 7)] * 3


def test_the_chain_declines_more_than_1000_utterances(dense):
    from ubisoft_laforge_daft_exprt_amd import ops
    assert ops.pitch_chain_applies(dense, torch.zeros(px.MAX_B, 80, 3), 'bf16')
    assert not ops.pitch_chain_applies(dense, torch.zeros(px.MAX_B + 1, 80, 3), 'bf16')
    assert not ops.pitch_chain_applies(dense, torch.zeros(4, 80, 3), 'f32')


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(px.EXACT_CASES))
def test_integer_network_is_exact_in_both_16_bit_types(name):
    """exact_reference asserts, for both modes, that rounding changes no tensor a kernel rounds and that all sums stay far below 2^24;
    here its statistics: the cases meet exact zeros (the strict > of the sign bits), both signs, and a gradient that is not sparse."""
    layers, mel, dpp, base, lens, rows_exist = px.exact_inputs(name)
    r = px.exact_reference(layers, mel, dpp, base, lens, rows_exist)
    s = r['stats']
    print(f'PITCH_EXACT_CPU case={name} ' + ' '.join(f'{k}={v:.3f}' for k, v in s.items()))
    assert s['act_max'] <= 256 and s['bwd_max'] <= 256
    assert s['zero'] >= 0.02 and s['pos'] >= 0.25 and s['neg'] >= 0.25 and s['dmel_nonzero'] >= 0.25, s
    for l in layers[:3]:
        assert bool((l['scale'] == 1).any()) and bool((l['scale'] == -1).any())
    v = px.valid_mask(lens, mel.shape[2], 'cpu')
    assert not dpp[~v].any() and (bool(v.all()) or bool((mel[(~v)[:, None, :].expand_as(mel)] != 0).any()))
    assert bool((base != 0).any())


def test_exact_cases_reach_the_edges_they_are_named_for():
    M, T, lens, _ = px.EXACT_CASES['many']
    tl = px.tiles(lens, T)
    assert len(lens) == 320 and len(tl) == 300 > px.MAX_GRID and any(n == 0 for n in lens[:64]) and any(n == 0 for n in lens[256:])
    M, T, lens, _ = px.EXACT_CASES['edges']
    assert {0, 1, 121, 122, 123, 243, 244, 245, 300} <= set(lens) and T == 300
    M, T, lens, ex = px.EXACT_CASES['rows_exist']
    assert all(a <= b for a, b in zip(lens, ex)) and any(a == b for a, b in zip(lens, ex)) and any(a < b for a, b in zip(lens, ex))
    assert len(px.EXACT_CASES['max_batch'][2]) == px.MAX_B


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_floor_constants_are_a_fresh_measurement(mode):
    fresh = px.measure_floor(mode)
    print(f'PITCH_FLOOR mode={mode} ' + ' '.join(f'{k}={v:.3e}' for k, v in fresh.items()))
    for k, v in fresh.items():
        assert v > 0 and 1.0 <= px.FLOOR[mode][k] / v <= 2.0, (k, v, px.FLOOR[mode][k])


@pytest.mark.parametrize('mode', MODES)
def test_few_sign_bits_sit_within_tau_of_zero(dense, refs, mode):
    cases, tau = refs[mode]
    assert all(t > 0 for t in tau)
    for name, ((mel, dpp, base, lens), r) in cases.items():
        share = px.mask_excluded(r, tau)
        print(f'PITCH_TAU mode={mode} case={name} tau={[f"{t:.2e}" for t in tau]} excluded={share:.4%}')
        assert share < px.MAX_MASK_EXCLUDED
        v = px.valid_mask(lens, mel.shape[2], 'cpu')
        assert bool((mel[(~v)[:, None, :].expand_as(mel)] != 0).all()) and not dpp[~v].any() and float((base != 0).float().mean()) > 0.999
    assert all(bool((l['scale'] > 0).any()) and bool((l['scale'] < 0).any()) for l in dense[:3])


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
def planted_figures(dense, refs, mode, plant):
    """the figures of the rounded tier's checks on the 'lengths' case when the 'device' is the restatement with one planted error"""
    cases, tau = refs[mode]
    (mel, dpp, base, lens), r = cases['lengths']
    B, M, T = mel.shape
    v = px.valid_mask(lens, T, 'cpu')
    v3 = v[:, None, :].expand(B, M, T)
    pp, pre = px.chain64(mel, dense, mode, lens, plant=plant)
    sg = px.signs64(pre, plant)                                                   # "the device's own masks"
    got = px.add_base(base, px.chain64_bwd(dpp, sg, dense, mode, plant=plant), lens)
    want = px.add_base(base, px.chain64_bwd(dpp, sg, dense, mode), lens)          # the test linearises at those masks
    wrong_bits = sum(int(((sg[l] != r['signs'][l]) & px.mask_clear(r, tau, l)[1]).sum()) for l in range(3))
    pmx, pmn = px.err_figures(pp, r['pp'], v)
    dmx, dmn = px.err_figures(got, want, v3)
    return {'pp_max': pmx, 'pp_mean': pmn, 'dmel_max': dmx, 'dmel_mean': dmn, 'wrong_bits': wrong_bits}


# plant -> the figures that must each sit at least 4 x over their bar
ROUNDED_PLANTS = {'halo': ('pp_max',), 'tile_off': ('pp_max', 'pp_mean'), 'drop_tap': ('pp_mean',),
                  'mask_word': ('dmel_max', 'dmel_mean'), 'trunc': ('pp_mean', 'dmel_mean')}


# (truncation is planted on bf16 alone, whose conversion is then a cut of the fp32 word)
@pytest.mark.parametrize('mode,plant', [(m, p) for p in ROUNDED_PLANTS for m in MODES if (m, p) != ('fp16', 'trunc')])
def test_planted_errors_break_the_rounded_tier(dense, refs, mode, plant):
    f = planted_figures(dense, refs, mode, plant)
    print(f'PITCH_PLANT mode={mode} plant={plant} ' + ' '.join(f'{k}={v / px.bar(mode, k):.1f}xbar' for k, v in f.items() if k != 'wrong_bits')
          + f' wrong_bits={f["wrong_bits"]}')
    for k in ROUNDED_PLANTS[plant]:
        assert f[k] >= 4 * px.bar(mode, k), (k, f[k], px.bar(mode, k))


def test_clean_restatement_has_no_wrong_bits_and_zero_figures(dense, refs):
    f = planted_figures(dense, refs, 'bf16', None)
    assert all(v == 0 for v in f.values()), f


@pytest.mark.parametrize('plant', ['halo', 'drop_tap', 'mask_word', 'tile_off', 'ge'])
def test_planted_errors_change_a_bit_of_the_exact_tier(plant):
    """(truncation cannot: the integer network has nothing to cut off, which is what makes it exact; the rounded tier sees it)"""
    layers, mel, dpp, base, lens, rows_exist = px.exact_inputs('edges')
    T = mel.shape[2]
    v = px.valid_mask(lens, T, 'cpu')
    clean = px.exact_reference(layers, mel, dpp, base, lens, rows_exist)
    pp, pre = px.chain64(mel, layers, 'bf16', lens, rows_exist, plant=plant)
    sg = px.signs64(pre, plant)
    dmel = px.add_base(base, px.chain64_bwd(dpp, clean['signs'], layers, 'bf16', rows_exist, plant=plant), lens)
    changed = {'pp': int((pp != clean['pp'])[v].sum()),
               'masks': sum(int((a != b)[v[:, None, :].expand_as(a)].sum()) for a, b in zip(sg, clean['signs'])),
               'dmel': int((dmel != clean['dmel']).sum())}
    print(f'PITCH_PLANT_EXACT plant={plant} changed={changed}')
    assert sum(changed.values()) > 0
    if plant == 'ge':
        assert changed['masks'] == sum(int((p == 0)[v[:, None, :].expand_as(p)].sum()) for p in clean['pre']) > 0
