"""CPU checks of the HiFi-GAN V2 and V3 generators' host side: the configuration whitelist, state-dict layouts against the reference
manifest, checkpoint forms, ``from_checkpoint``, the plain-torch restatement against the reference fixture, the zero padding of V2's
8-channel stage, the streaming plan run in float64, and the argument checks of the new entry points."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import vocoder_helpers as vh
from tests import vocoder_torch as vt
from tests.vocoder_stream_helpers import emulate, simulate
from ubisoft_laforge_daft_exprt_amd import vocoder as voc

CONFIGS = {'v1': voc.v1_config, 'v2': voc.v2_config, 'v3': voc.v3_config}
LENGTHS = (1, 13, 40)


def test_check_config_is_a_whitelist_of_three():
    for name, make in CONFIGS.items():
        cfg = make()
        assert voc.check_config(cfg) == cfg
        as_tuples = {k: (tuple(tuple(x) if isinstance(x, list) else x for x in v) if isinstance(v, list) else v) for k, v in cfg.items()}
        assert isinstance(as_tuples['upsample_rates'], tuple) and isinstance(as_tuples['resblock_dilation_sizes'][0], tuple)
        assert voc.check_config(as_tuples) == as_tuples
        assert voc.HiFiGANGenerator(as_tuples).config == as_tuples
    assert voc.check_config(None) == voc.v1_config() == voc.DEFAULT_CONFIG
    for key, value in (('resblock', '2'), ('upsample_rates', [8, 8, 4]), ('upsample_initial_channel', 256), ('upsample_rates', [8, 8, 4, 2])):
        cfg = copy.deepcopy(voc.v1_config())
        cfg[key] = value
        with pytest.raises(NotImplementedError, match='V1.*V2.*V3'):
            voc.check_config(cfg)
        with pytest.raises(NotImplementedError):
            voc.stream_plan(cfg, 8)
    assert voc.workspace_bytes_per_frame(None) == voc.workspace_bytes_per_frame(voc.v1_config()) == voc.WORKSPACE_BYTES_PER_FRAME == 163840
    assert voc.workspace_bytes_per_frame(voc.v2_config()) == 5 * 4096 * 4       # 16 padded channels x 256 samples per frame
    assert voc.workspace_bytes_per_frame(voc.v3_config()) == 5 * 8192 * 4


@pytest.mark.parametrize('name', vh.VARIANTS)
def test_state_dict_keys_and_shapes_match_reference_manifest(name):
    man = vh.manifest(name)
    assert CONFIGS[name]() == man['config']
    gen = voc.HiFiGANGenerator(CONFIGS[name]())
    sd = gen.state_dict()
    assert sorted(sd) == sorted(man['keys']) and len(sd) == {'v2': 234, 'v3': 69}[name]
    for k, shape in man['keys'].items():
        assert list(sd[k].shape) == shape, k
    gen.load_state_dict(vh.state_dict(name), strict=True)
    assert list(sd['conv_post.weight_v'].shape) == [1, {'v2': 8, 'v3': 32}[name], 7]       # the checkpoint's width, not the padded one


@pytest.mark.parametrize('name', vh.VARIANTS)
def test_every_checkpoint_form_loads_the_same_folded_weights(name, tmp_path):
    sd, cfg = vh.state_dict(name), CONFIGS[name]()
    plain_vocoder = voc.HiFiGanVocoder(sd, config=cfg, device='cpu')
    plain = plain_vocoder.weights
    assert all(torch.equal(v, sd[k]) for k, v in plain_vocoder.generator.state_dict().items())
    folded_sd = {}
    for layer, (w, b) in plain.items():
        folded_sd[layer + '.weight'], folded_sd[layer + '.bias'] = w, b
    for i, form in enumerate([{'generator': sd}, {'state_dict': sd}, sd, {'generator': folded_sd}, folded_sd]):
        path = os.path.join(str(tmp_path), f'g{i}.pth')
        torch.save(form, path)
        for loaded in (voc.HiFiGanVocoder(path, config=cfg, device='cpu'), voc.HiFiGanVocoder.from_checkpoint(path, device='cpu')):
            assert loaded.config == cfg
            assert (loaded.generator is None) == (form is folded_sd or form.get('generator') is folded_sd)
            assert sorted(loaded.weights) == sorted(plain)
            for k in plain:
                assert torch.equal(loaded.weights[k][0], plain[k][0]) and torch.equal(loaded.weights[k][1], plain[k][1]), (i, k)
    # strict: under the V1 configuration a V2 checkpoint has the wrong shapes and a V3 checkpoint lacks layers
    with pytest.raises(RuntimeError if name == 'v2' else KeyError):
        voc.HiFiGanVocoder(sd, config=None, device='cpu')
    with pytest.raises(KeyError, match='conv_post'):
        voc.HiFiGanVocoder({k: v for k, v in sd.items() if not k.startswith('conv_post')}, config=cfg, device='cpu')


def test_from_checkpoint_picks_the_configuration_from_the_shapes():
    for name, make in CONFIGS.items():
        v = voc.HiFiGanVocoder.from_checkpoint(vh.state_dict(name), device='cpu', precision='bf16')
        assert v.config == make() and v.precision == 'bf16' and v.generator is not None
    sd = vh.state_dict('v1')
    wide = dict(sd)
    for k in ('conv_pre.bias', 'conv_pre.weight_g', 'conv_pre.weight_v'):
        wide[k] = torch.zeros(384, *sd[k].shape[1:])
    with pytest.raises(NotImplementedError, match='384'):
        voc.HiFiGanVocoder.from_checkpoint(wide, device='cpu')
    three = {k: v for k, v in sd.items() if not k.startswith('ups.3.')}                   # V1's width with three upsampling stages
    with pytest.raises(NotImplementedError):
        voc.HiFiGanVocoder.from_checkpoint(three, device='cpu')
    with pytest.raises(ValueError, match='checkpoint_path'):
        voc.HiFiGanVocoder.from_checkpoint(None)
    with pytest.raises(ValueError, match='precision'):
        voc.stream_plan(voc.v3_config(), 8, 'fp16')
    assert voc.load_hifigan_vocoder(sd, device='cpu').config == voc.v1_config()           # the reference's helper still means V1


@pytest.mark.parametrize('name', ['v1', 'v2', 'v3'])
def test_torch_restatement_matches_reference_golden(name):
    cfg = CONFIGS[name]()
    if name == 'v1':
        lengths, mels, wavs = vh.golden()
    else:
        gold = vh.variant_golden(name)
        lengths, mels, wavs = gold['lengths'], gold['mels'], gold['wavs']
        assert max(gold['f32_max']) <= 2e-6 and max(gold['f32_mean']) <= 3e-7             # the reference's own fp32 spread, as V1's
    weights = voc.fold_state_dict(vh.state_dict(name), voc.HiFiGANGenerator(cfg).layer_names())
    for n, mel, ref in zip(lengths, mels, wavs):
        with torch.no_grad():
            got = vt.generator(torch.from_numpy(mel)[None], weights, cfg)[0].numpy()
        assert got.shape == (256 * n,)
        assert np.abs(got - ref).max() <= 1e-5, n


def test_padded_v2_stage_is_exactly_zero_and_changes_nothing_in_float64():
    cfg = voc.v2_config()
    folded = voc.fold_state_dict(vh.state_dict('v2'), voc.HiFiGANGenerator(cfg).layer_names())
    padded = voc.pad_folded_weights(folded, cfg)
    assert sorted(padded) == sorted(folded)
    last = [n for n in folded if n.startswith('resblocks.') and int(n.split('.')[1]) >= 9]
    assert len(last) == 18
    for n in folded:
        (w, b), (pw, pb) = folded[n], padded[n]
        if n == 'ups.3':
            assert pw.shape == (16, 16, 4) and pb.shape == (16,) and torch.equal(pw[:, :8], w) and torch.equal(pb[:8], b)
            assert not pw[:, 8:].any() and not pb[8:].any()
        elif n in last:
            assert pw.shape == (16, 16, w.shape[2]) and pb.shape == (16,) and torch.equal(pw[:8, :8], w) and torch.equal(pb[:8], b)
            assert not pw[8:].any() and not pw[:, 8:].any() and not pb[8:].any()
        elif n == 'conv_post':
            assert pw.shape == (1, 16, 7) and torch.equal(pw[:, :8], w) and not pw[:, 8:].any() and torch.equal(pb, b)
        else:
            assert pw is w and pb is b, n
    for make in (voc.v1_config, voc.v3_config):                        # nothing to pad
        f = voc.fold_state_dict(vh.state_dict('v1' if make is voc.v1_config else 'v3'), voc.HiFiGANGenerator(make()).layer_names())
        assert all(voc.pad_folded_weights(f, make())[n][0] is f[n][0] for n in f)
    mel = torch.from_numpy(vh.variant_golden('v2')['mels'][2])[None].double()
    with torch.no_grad():
        a = vt.generator(mel, vt.to(folded, 'cpu', torch.float64), cfg)
        b = vt.generator(mel, vt.to(padded, 'cpu', torch.float64), cfg)
    assert (a - b).abs().max().item() <= 1e-12


# ---- the streaming plan in float64 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=vh.VARIANTS)
def variant64(request):
    """(name, config, float64 weights as the kernels run them (padded), the mel, {length: the whole generator's waveform})"""
    name = request.param
    cfg = CONFIGS[name]()
    folded = voc.fold_state_dict(vh.state_dict(name), voc.HiFiGANGenerator(cfg).layer_names())
    W = vt.to(voc.pad_folded_weights(folded, cfg), 'cpu', torch.float64)
    mel = torch.from_numpy(vh.variant_golden(name)['mels'][2])[None].double()
    with torch.no_grad():
        return name, cfg, W, mel, {n: vt.generator(mel[:, :, :n], W, cfg)[0] for n in LENGTHS}


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('chunk_frames', [1, 4, 32])
def test_stream_plan_bookkeeping_and_schedule_in_float64(variant64, chunk_frames, precision):
    name, cfg, W, mel, refs = variant64
    plan = voc.stream_plan(cfg, chunk_frames, precision)
    kinds = [ln['kind'] for ln in plan.launches]
    if name == 'v2':
        assert len(kinds) == 42 and kinds.count('pair') == 36 and plan.tensors['sum.3']['channels'] == 16
    else:
        n_chain = len([1 for c in (64, 32) for k in (3, 5, 7) if (precision, c, k) in voc.CHAIN_SHAPES])
        assert n_chain == (4 if precision == 'bf16' else 0)             # the fused ResBlock2 is the launch path under bf16 at widths 3 and 5
        assert kinds.count('chain') == n_chain and len(kinds) == 23 - n_chain and 'pair' not in kinds
        for ln in plan.launches:
            if ln['kind'] == 'chain':
                assert ln['left'] == ln['right'] == (ln['dil'] + ln['dil2']) * (ln['taps'] - 1) // 2
    assert kinds[-1] == 'post' and plan.launches[-1]['cin'] == {'v2': 16, 'v3': 32}[name]
    for tname, t in plan.tensors.items():
        assert t['ring'] & (t['ring'] - 1) == 0 and t['ring'] >= chunk_frames * t['scale'] + t['lag'] and t['lag'] >= 0, tname
    assert all(ln['lag'] >= 0 for ln in plan.launches)
    assert {n: t['lag'] for n, t in plan.tensors.items()} == {n: t['lag'] for n, t in voc.stream_plan(cfg, 8, precision).tensors.items()}
    for length in LENGTHS:
        simulate(plan, length)
        with torch.no_grad():
            got = emulate(plan, mel[:, :, :length], length, W)
        ref = refs[length]
        assert got.shape[0] == -(-length // chunk_frames) * chunk_frames * voc.HOP
        err = (got[:ref.shape[0]] - ref).abs().max().item()
        print(f'{name} length {length}, chunks of {chunk_frames}: max abs {err:.2e}')
        assert err <= 1e-12
        assert torch.count_nonzero(got[ref.shape[0]:]).item() == 0


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import lib, DxError
    L = lib()
    chain = lambda X=4096, Y=8192, W1=1, C=64, taps=7, d1=3, d2=12: L.dx_voc_chain(X, C * 8, W1, 1, 1, 1, Y, 1, 1, 1, 8, C, taps, d1, d2, 0, 0, None)
    with pytest.raises(DxError, match='null'):
        chain(W1=None)
    with pytest.raises(DxError, match='alias'):
        chain(Y=4096)
    with pytest.raises(DxError, match='aligned'):
        chain(X=4100)
    for bad in (dict(C=16), dict(C=128), dict(C=48)):
        with pytest.raises(DxError, match='C in'):
            chain(**bad)
    for bad in (dict(taps=9), dict(taps=4), dict(d1=4), dict(d2=13), dict(d1=0), dict(taps=3, d2=37)):
        with pytest.raises(DxError, match='taps'):
            chain(**bad)
    win = lambda **k: L.dx_voc_chain_win(4096, 64 * 8, 1, 1, 1, 1, 8192, 64 * 8, 1, 1, 1, 8, 64, 7, 3, 12, 0, 0,
                                         k.get('cursor', 16), k.get('step', 4), 0, k.get('mx', 7), k.get('my', 7), None)
    with pytest.raises(DxError, match='window'):
        win(cursor=None)
    with pytest.raises(DxError, match='window'):
        win(mx=6)
    with pytest.raises(DxError, match='ring'):
        win(my=15)
    post = lambda X=4096, W=1, C=16: L.dx_voc_post_c(X, C * 8, W, 1, 8192, 8, 1, 1, 1, 8, 8, C, None)
    with pytest.raises(DxError, match='null'):
        post(W=None)
    with pytest.raises(DxError, match='aligned'):
        post(X=4100)
    for C in (8, 24, 64):
        with pytest.raises(DxError, match='channel'):
            post(C=C)
    with pytest.raises(DxError, match='channel'):
        L.dx_voc_post_c_win(4096, 16 * 8, 1, 1, 8192, 8, 1, 1, 1, 8, 8, 8, 16, 4, 0, 7, 0, None)
    with pytest.raises(DxError, match='chunk buffer'):
        L.dx_voc_post_c_win(4096, 16 * 8, 1, 1, 8192, 8, 1, 1, 1, 8, 8, 16, 16, 4, 0, 7, 7, None)
    with pytest.raises(DxError, match='bad shape'):                     # the ring of 16 rows of 16 channels does not fit the batch stride
        L.dx_voc_post_c_win(4096, 16 * 8, 1, 1, 8192, 8, 1, 1, 1, 8, 8, 16, 16, 4, 0, 15, 0, None)
    # the widened checks of the old entry points: 16 columns pass the shape check (the next check, aliasing, is the one that fires) ...
    conv = lambda Cout=16, taps=3, dil=1, Y=4096: L.dx_voc_conv(4096, 64 * 8, 64, 1, 1, None, Y, Cout * 8, None, 1, 1, 1, 8, 64, Cout, taps, dil, 1, 1, 0, 0, None)
    for ok in (dict(Cout=16), dict(taps=7, dil=12), dict(taps=5, dil=6), dict(taps=11, dil=5)):
        with pytest.raises(DxError, match='alias'):
            conv(**ok)
    # ... and what is still out of range does not
    with pytest.raises(DxError, match='Cout'):
        conv(Cout=8)
    for bad in (dict(taps=7, dil=13), dict(taps=11, dil=8), dict(taps=13), dict(dil=0)):
        with pytest.raises(DxError, match='taps'):
            conv(**bad)
    pair = lambda C=16, taps=3, dil=1, Y=4096: L.dx_voc_pair(4096, C * 8, 1, 1, 1, 1, Y, 1, 1, 1, 8, C, taps, dil, 0, 0, None)
    with pytest.raises(DxError, match='alias'):
        pair()
    with pytest.raises(DxError, match='C in'):
        pair(C=8, Y=8192)
    with pytest.raises(DxError, match='taps'):
        pair(taps=5, Y=8192)


def test_new_entry_points_are_priced():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[5, 9, 12]])
    a = dict(B=3, N=96, scale=8, C=64, taps=7, d1=3, d2=12, bf16=0, acc_mode=2, step=32, lag=10)
    label, bound, flops, byt = profiling.price('dx_voc_chain', a, geom)
    assert (label, bound) == ('voc_chain<f32>', 'mfma') and flops == 2.0 * 2 * 7 * 64 * 64 * (5 + 9 + 12) * 8
    assert byt == (5 + 9 + 12) * 8 * 64 * 4 * 3
    assert profiling.price('dx_voc_chain_win', a, geom)[2] == 2.0 * 2 * 7 * 64 * 64 * (3 * 32)
    p = dict(B=3, N=96, scale=8, C=16, ncols=96)
    assert profiling.price('dx_voc_post_c', p, geom) == ('voc_post', 'hbm', None, (5 + 9 + 12) * 8 * 16 * 4 + 3 * 96 * 4)
    assert profiling.price('dx_voc_post_c_win', dict(p, step=32, lag=3), geom)[3] == 3 * 32 * 16 * 4 + 3 * 96 * 4
