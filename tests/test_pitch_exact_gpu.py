"""The fused pitch-predictor chain (csrc/dx_pitch.hip: dx_pitch_chain_fwd / _bwd and their _f16 twins) against float64, in two tiers
(tests/pitch_exact_helpers.py states the restatement, the inputs and the bars; tests/test_pitch_exact_cpu.py tests that statement).

EXACT: an integer-valued network, every intermediate exactly representable, so pp, every contracted sign bit and dmel must equal float64
bit for bit, and every element the launches must not write keeps its bits.  ROUNDED: a dense random network against float64 that rounds
where the kernels round, under bars of 4 x the restatement's own spread over fp32 summation orders.  The C entries are called directly,
on buffers of the test's own: pp pre-filled with a sentinel, the sign words with random bits, dmel with a nonzero base.

Measured on the MI355X (worst ratio of a figure to its bar over the cases; DESIGN.md, "The pitch chain against float64"):
                    pp max   pp mean   dmel max   dmel mean   sign bits wrong outside tau   farthest flip
  exact, 7 cases    bitwise in both modes (pp, sign words, dmel, and everything that must stay untouched)
  rounded, bf16     0.26     0.65      0.20       0.16        0 of 0.66 M / 1.52 M          0.25 tau
  rounded, fp16     0.14     0.32      0.20       0.23        0 of 0.66 M / 1.52 M          0.82 tau
The device's fp32 accumulation noise (median pp error 2-4e-7) is 2-3 x that of the restatement's orders (one rounding per K step), and
the 16-bit rounding flips that make up the mean grow with it: hence 0.65 and not 0.25.
"""
import pytest
import torch

from tests import pitch_exact_helpers as px

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MODES = ['bf16', 'fp16']
SENTINEL = -12345.5


@pytest.fixture(scope='module')
def ops():
    from ubisoft_laforge_daft_exprt_amd import ops as _ops
    _ops.set_precision('f32')
    return _ops


def i32(vals):
    return None if vals is None else torch.tensor(vals, dtype=torch.int32, device=DEV)


def random_words(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31, shape, generator=g, device=DEV, dtype=torch.int64).to(torch.int32)


def attach_packs(ops, layers):
    for l in layers:
        l['pack'] = ops.PackedWeight(l['w'])
    return layers


def entry(name, mode):
    from ubisoft_laforge_daft_exprt_amd import _lib
    return getattr(_lib.lib(), name + ('_f16' if mode == 'fp16' else ''))


def stream():
    return torch.cuda.current_stream().cuda_stream


def launch_fwd(layers, mode, mel, lens, rows_exist, pp, masks):
    B, M, T = mel.shape
    assert mel.is_contiguous() and pp.shape == (B, T) and masks.shape == (B, T, 3, 8) and lens.numel() == B
    img = [l['pack'].image(mode) for l in layers[:3]]
    p = lambda t: None if t is None else t.data_ptr()
    entry('dx_pitch_chain_fwd', mode)(p(mel), B, M, T, p(lens), p(img[0].fwd), p(img[1].fwd), p(img[2].fwd),
                                      p(layers[0]['b']), p(layers[1]['b']), p(layers[2]['b']),
                                      p(layers[0]['scale']), p(layers[1]['scale']), p(layers[2]['scale']),
                                      p(layers[0]['shift']), p(layers[1]['shift']), p(layers[2]['shift']),
                                      p(layers[3]['w']), float(layers[3]['b3']), p(pp), p(masks), p(rows_exist), stream())


def launch_bwd(layers, mode, dpp, lens, rows_exist, masks, dmel):
    B, M, T = dmel.shape
    assert dmel.is_contiguous() and dpp.is_contiguous() and dpp.shape == (B, T) and masks.shape == (B, T, 3, 8)
    img = [l['pack'].image(mode) for l in layers[:3]]
    p = lambda t: None if t is None else t.data_ptr()
    entry('dx_pitch_chain_bwd', mode)(p(dpp), B, M, T, p(lens), p(img[0].bwd), p(img[1].bwd), p(img[2].bwd),
                                      p(layers[0]['scale']), p(layers[1]['scale']), p(layers[2]['scale']),
                                      p(layers[3]['w']), p(masks), p(dmel), p(rows_exist), stream())


def run(layers, mode, mel, dpp, base, lens, rows_exist=None, seed=11, scramble=False):
    """one forward and one backward launch on fresh buffers -> (pp, masks as the forward left them, dmel).  ``scramble``: the sign words
    of frames at or past rows_exist are overwritten with random bits between the two launches."""
    B, M, T = mel.shape
    L, E = i32(lens), i32(rows_exist)
    pp = torch.full((B, T), SENTINEL, device=DEV)
    masks = random_words((B, T, 3, 8), seed)
    launch_fwd(layers, mode, mel.contiguous(), L, E, pp, masks)
    fed = masks.clone()
    if scramble:
        gone = ~px.exist_mask(B, T, rows_exist, DEV)
        fed[gone] = random_words((B, T, 3, 8), seed + 1)[gone]
    dmel = base.clone()
    launch_bwd(layers, mode, dpp.contiguous(), L, E, fed, dmel)
    torch.cuda.synchronize()
    return pp, masks, dmel


def count(t):
    return int(t.sum())


# ---- exact tier -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def exact_refs():
    """case -> (inputs on the device, float64 results): computed once, shared by both modes, never modified"""
    cache = {}

    def get(name):
        if name not in cache:
            inputs = px.exact_inputs(name, device=DEV)
            cache[name] = (inputs, px.exact_reference(*inputs))
        return cache[name]
    return get


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(px.EXACT_CASES))
def test_integer_network_is_bitwise_float64(ops, exact_refs, name, mode):
    (layers, mel, dpp, base, lens, rows_exist), ref = exact_refs(name)
    if 'pack' not in layers[0]:
        attach_packs(ops, layers)
    B, M, T = mel.shape
    assert ops.pitch_chain_applies(layers, mel, mode)
    mel_in, dpp_in = mel, dpp
    if rows_exist is not None:                                  # what lies at or past rows_exist is not there: NaN in, nothing out
        gone = ~px.exist_mask(B, T, rows_exist, DEV)
        mel_in, dpp_in = mel.clone(), dpp.clone()
        mel_in[gone[:, None, :].expand_as(mel)] = float('nan')
        dpp_in[gone] = float('nan')
    pp, masks, dmel = run(layers, mode, mel_in, dpp_in, base, lens, rows_exist, scramble=rows_exist is not None)
    v = px.valid_mask(lens, T, DEV)
    want_pp = torch.where(v, ref['pp'].float(), torch.full_like(pp, SENTINEL))
    bad_pp = count(~px.bits_equal(pp, want_pp))
    dec = px.signs_of(masks)
    bad_bits = checked = 0
    for l in range(3):
        region = px.mask_check_region(l, lens, T, rows_exist, DEV)[:, None, :].expand_as(dec[l])
        bad_bits += count((dec[l] != ref['signs'][l]) & region)
        checked += count(region)
    bad_dmel = count(~px.bits_equal(dmel, ref['dmel'].float()))
    untouched = count(~px.bits_equal(dmel, base) & ~v[:, None, :].expand_as(dmel))
    print(f'PITCH_EXACT case={name} mode={mode} tiles={len(px.tiles(lens, T))} pp_wrong={bad_pp}/{pp.numel()} '
          f'mask_bits_wrong={bad_bits}/{checked} dmel_wrong={bad_dmel}/{dmel.numel()} dmel_written_past_len={untouched}')
    assert bad_pp == 0 and bad_bits == 0 and bad_dmel == 0 and untouched == 0
    assert checked > 0 and bool((dmel != base).any())


# ---- rounded tier -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dense(ops):
    return px.dense_layers(DEV, ops.DEFAULT)


@pytest.fixture(scope='module')
def rounded_refs(dense):
    """(case, mode) -> (inputs on the device, float64 results, tau of the mode, the device's results): computed once, never modified"""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            per_case = {}
            for n in px.ROUNDED_CASES:
                inputs = px.rounded_inputs(n, DEV)
                per_case[n] = (inputs, px.rounded_reference(dense, *inputs, mode))
            tau = px.mask_tau([r for _, r in per_case.values()])
            for n, (inputs, ref) in per_case.items():
                cache[n, mode] = (inputs, ref, tau, run(dense, mode, *inputs))
        return cache[name, mode]
    return get


def ratios(mode, **figures):
    return {k: v / px.bar(mode, k) for k, v in figures.items()}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(px.ROUNDED_CASES))
def test_dense_network_stays_within_four_noise_floors(ops, dense, rounded_refs, name, mode):
    (mel, dpp, base, lens), ref, tau, (pp, masks, dmel) = rounded_refs(name, mode)
    B, M, T = mel.shape
    assert ops.pitch_chain_applies(dense, mel, mode)
    v = px.valid_mask(lens, T, DEV)
    v3 = v[:, None, :].expand(B, M, T)
    # forward
    assert bool((pp[~v] == SENTINEL).all()) and bool(torch.isfinite(pp).all())
    pmx, pmn = px.err_figures(pp, ref['pp'], v)
    # sign bits, wherever float64 is clearly away from zero
    dec = px.signs_of(masks)
    bad_bits = checked = 0
    worst_wrong = 0.0                                    # the largest |v64| / tau at which a device bit differs from float64's
    for l in range(3):
        region, clear = px.mask_clear(ref, tau, l)
        wrong = (dec[l] != ref['signs'][l]) & region
        if bool(wrong.any()):
            worst_wrong = max(worst_wrong, float(ref['pre'][l][wrong].abs().max()) / tau[l])
        bad_bits += count(wrong & clear)
        checked += count(clear)
    excluded = px.mask_excluded(ref, tau)
    # backward, linearised at the device's own sign bits
    want = px.add_base(base, px.chain64_bwd(dpp, dec, dense, mode), lens)
    dmx, dmn = px.err_figures(dmel, want, v3)
    past = count(~px.bits_equal(dmel, base) & ~v3)
    r = ratios(mode, pp_max=pmx, pp_mean=pmn, dmel_max=dmx, dmel_mean=dmn)
    print(f'PITCH_ROUNDED case={name} mode={mode} ' + ' '.join(f'{k}={x:.3f}xbar' for k, x in r.items())
          + f' mask_bits_wrong={bad_bits}/{checked} farthest_flip={worst_wrong:.3f}xtau excluded={excluded:.4%} dmel_written_past_len={past}')
    assert excluded < px.MAX_MASK_EXCLUDED
    assert bad_bits == 0
    assert past == 0 and bool(torch.isfinite(dmel).all())
    assert all(x < 1.0 for x in r.values()), r


@pytest.mark.parametrize('mode', MODES)
def test_a_second_launch_gives_the_same_bits(dense, rounded_refs, mode):
    for name in px.ROUNDED_CASES:
        (mel, dpp, base, lens), ref, tau, (pp, masks, dmel) = rounded_refs(name, mode)
        pp2, masks2, dmel2 = run(dense, mode, mel, dpp, base, lens, seed=12)       # other bits under the words no launch writes
        T = mel.shape[2]
        written = torch.stack([px.mask_check_region(l, lens, T, None, DEV) for l in range(3)], dim=2)[..., None].expand_as(masks)
        assert bool(px.bits_equal(pp, pp2).all()) and bool(px.bits_equal(dmel, dmel2).all()) and bool((masks == masks2)[written].all())


@pytest.mark.parametrize('mode', MODES)
def test_rows_of_a_large_batch_equal_the_rows_launched_alone(dense, rounded_refs, mode):
    """300 tiles on 256 workgroups, a tile prefix over five 64-lane blocks: the utterances at the block borders and the ones whose
    workgroup runs a second tile give the bits they give as a batch of one."""
    (mel, dpp, base, lens), ref, tau, (pp, masks, dmel) = rounded_refs('many', mode)
    T = mel.shape[2]
    for b in px.MANY_ALONE:
        n = lens[b]
        assert n > 0
        pp1, masks1, dmel1 = run(dense, mode, mel[b:b + 1], dpp[b:b + 1], base[b:b + 1], [n], seed=100 + b)
        assert bool(px.bits_equal(pp1[0, :n], pp[b, :n]).all()), b
        assert bool((masks1[0, :n] == masks[b, :n]).all()), b
        assert bool(px.bits_equal(dmel1[0], dmel[b]).all()), b


@pytest.mark.parametrize('mode', MODES)
def test_a_mel_frame_reaches_four_frames_each_way_and_no_further(dense, rounded_refs, mode):
    """frame 118 is the first halo frame of the second tile (its window starts at 122 - 4), 121 its last, 122 its first own frame.  The
    changed batch meets the forward bars as a whole (the mean's floor was measured over all valid frames of the case, not over one row)."""
    (mel, dpp, base, lens), ref, tau, (pp0, _, _) = rounded_refs('lengths', mode)
    b = lens.index(300)
    T = mel.shape[2]
    v = px.valid_mask(lens, T, DEV)
    others = torch.arange(len(lens), device=DEV) != b
    worst = {}
    for n in (118, 121, 122):
        m2 = mel.clone()
        m2[b, 17, n] += 1.0
        pp1 = run(dense, mode, m2, dpp, base, lens)[0]
        same = px.bits_equal(pp1, pp0)
        assert bool(same[others].all()) and bool(same[b, :n - 4].all()) and bool(same[b, n + 5:].all()), n
        assert count(~same[b, n - 4:n + 5]) >= 5, n
        want, _ = px.chain64(m2, dense, mode, lens)
        mx, mn = px.err_figures(pp1, want, v)
        r = ratios(mode, pp_max=mx, pp_mean=mn)
        worst = {k: max(worst.get(k, 0.0), x) for k, x in r.items()}
        assert all(x < 1.0 for x in r.values()), (n, r)
    print(f'PITCH_LOCAL mode={mode} ' + ' '.join(f'{k}={x:.3f}xbar' for k, x in worst.items()))
