"""CPU checks of the prosody-transfer path: the three entry points are declared and exported, arguments are checked before any
launch, the host side of ``condition_external_prosody`` (speaker statistics, durations with alpha_dur) equals the reference golden, and
the float64 restatements of tests/prosody_helpers.py reproduce tests/golden/prosody.npz within its stored spread."""
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers
from tests import prosody_helpers as ph
from ubisoft_laforge_daft_exprt_amd import _lib, speech

ENTRIES = ('dx_symbol_prosody', 'dx_prosody_condition', 'dx_pcm16')


@pytest.fixture(scope='module')
def g():
    return ph.golden()


def test_entries_are_declared_exported_and_public():
    import ubisoft_laforge_daft_exprt_amd as dx
    protos = _lib.parse_header(with_names=True)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos and hasattr(dll, name), name
        assert protos[name][2][-1] == 'stream'
    assert protos['dx_pcm16'][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
    for name in ('SpeechSynthesizer', 'condition_external_prosody', 'symbol_prosody', 'to_pcm16'):
        assert getattr(dx, name) is getattr(speech, name)


def test_bad_arguments_raise_before_any_launch():
    L, E = _lib.lib(), _lib.DxError
    p = 4096                                                  # any non-null, 16-byte aligned value: the checks fail before it is used
    with pytest.raises(E, match='null'):
        L.dx_symbol_prosody(None, p, 8, p, p, p, p, 1, 8, 4, None)
    with pytest.raises(E, match='null'):
        L.dx_symbol_prosody(p, p, 8, p, p, p, None, 1, 8, 4, None)
    for B, T, Lx, ldt in ((0, 8, 4, 8), (-1, 8, 4, 8), (1, -1, 4, 8), (1, 8, 0, 8), (1, 8, -3, 8), (1, 8, 4, 7)):
        with pytest.raises(E, match='bad sizes'):
            L.dx_symbol_prosody(p, p, ldt, p, p, p, p, B, T, Lx, None)
    cond = lambda **kw: L.dx_prosody_condition(*[{**dict(energy=p, pitch=p, dur_int=p, in_lens=p, ef=p, pf=p, stats=p, source=None, has_source=0, ae=1.0,
                                                          ap=1.0, mode=1, normalize=1, eo=p, po=p, B=2, L=5, stream=None), **kw}[k]
                                                 for k in ('energy', 'pitch', 'dur_int', 'in_lens', 'ef', 'pf', 'stats', 'source', 'has_source', 'ae', 'ap',
                                                           'mode', 'normalize', 'eo', 'po', 'B', 'L', 'stream')])
    for kw in (dict(energy=None), dict(pitch=None), dict(in_lens=None), dict(eo=None), dict(po=None)):
        with pytest.raises(E, match='null'):
            cond(**kw)
    for kw in (dict(B=0), dict(B=-2), dict(L=0), dict(L=-1)):
        with pytest.raises(E, match='bad sizes'):
            cond(**kw)
    with pytest.raises(E, match='mode'):
        cond(mode=3)
    with pytest.raises(E, match='pitch_factors'):
        cond(pf=None, mode=2)
    with pytest.raises(E, match='stats'):
        cond(stats=None)
    with pytest.raises(E, match='stats'):
        cond(stats=None, normalize=0, mode=1)
    with pytest.raises(E, match='has_source'):
        cond(has_source=1)
    with pytest.raises(E, match='null'):
        L.dx_pcm16(None, p, p, 1, 8, None)
    with pytest.raises(E, match='null'):
        L.dx_pcm16(p, p, None, 1, 8, None)
    for B, S in ((0, 8), (-1, 8), (1, 0), (1, -8), (65536, 8)):
        with pytest.raises(E, match='bad sizes'):
            L.dx_pcm16(p, p, p, B, S, None)
    with pytest.raises(E, match='aligned'):
        L.dx_pcm16(p + 4, p, p, 1, 8, None)


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError, match='GPU'):
        speech.symbol_prosody(torch.zeros(1, 4), torch.zeros(1, 4), torch.ones(1, 2, dtype=torch.long), torch.tensor([2]))
    with pytest.raises(RuntimeError, match='GPU'):
        speech.to_pcm16(torch.zeros(1, 8), [8])
    hp = helpers.golden_hparams(stats=helpers.FEATURE_STATS)
    with pytest.raises(RuntimeError, match='GPU'):
        speech.condition_external_prosody([{'durations_frames': [1.0], 'energy': [1.0], 'pitch': [1.0]}], [0], hp, device='cpu')


def test_speaker_statistics_lookup_and_its_errors(g):
    hp = helpers.golden_hparams(stats=ph.stats_dict(g))
    table = speech.speaker_stats_table(torch.from_numpy(g['cond/speaker_ids']), hp)
    assert table.dtype == torch.float32 and np.array_equal(table.numpy(), ph.stats_rows(g).astype(np.float32))
    assert np.array_equal(table[2].numpy(), table[0].numpy())                     # speaker 5 took 'spk 0'
    entry = [{'durations_frames': [3.0, 2.0], 'energy': [1.0, 0.0], 'pitch': [5.0, 0.0]}]
    no_fallback = helpers.golden_hparams(stats={'spk 1': ph.stats_dict(g)['spk 1']})
    with pytest.raises(KeyError, match="spk 7"):
        speech.condition_external_prosody(entry, [7], no_fallback)
    for feature in ('energy', 'pitch'):
        st = ph.stats_dict(g)
        st['spk 1'][feature]['std'] = 0.0
        with pytest.raises(ValueError, match='not initialized'):
            speech.condition_external_prosody(entry, [1], helpers.golden_hparams(stats=st))
        src = ph.source_dict(g)
        src[feature]['std'] = 0
        with pytest.raises(ValueError, match='Source stats'):
            speech.condition_external_prosody(entry, [0], hp, source_stats=src)
    assert np.array_equal(speech.source_stats_row(ph.source_dict(g)).numpy(), g['cond/source_stats'].astype(np.float32))
    assert speech.source_stats_row(None) is None


@pytest.mark.parametrize('alpha_dur', [1.0, 1.3, 0.5])
def test_host_durations_equal_the_reference_exactly(g, alpha_dur):
    hp = helpers.golden_hparams()
    frames, lens = g['cond/durations_frames'], g['cond/in_lens']
    seconds, ints = g[f'dur/a{alpha_dur}/seconds'], g[f'dur/a{alpha_dur}/int']
    assert seconds.dtype == np.float32 and ints.dtype == np.int64
    for b, n in enumerate(lens):
        s, i = speech.host_durations(frames[b, :n].tolist(), alpha_dur, hp)
        assert s.dtype == torch.float32 and i.dtype == torch.long
        assert np.array_equal(s.numpy(), seconds[b, :n]) and np.array_equal(i.numpy(), ints[b, :n]), (alpha_dur, b)
        assert not seconds[b, n:].any() and not ints[b, n:].any()
    assert np.array_equal(frames, g['cond/durations_frames'])                    # the caller's durations are left alone
    if alpha_dur != 1.0:
        assert not np.array_equal(ints, g['dur/a1.0/int'])


def test_symbol_mean_restatement_reproduces_the_golden(g):
    e64, p64 = ph.symbol_means64(g['sym/frames_energy'], g['sym/frames_pitch'], g['sym/dur_int'], g['sym/in_lens'])
    assert np.array_equal(e64, g['sym/energy_f64']) and np.array_equal(p64, g['sym/pitch_f64'])
    s = g['sym/spread']
    de, dp = np.abs(g['sym/energy_ref32'] - e64), np.abs(g['sym/pitch_ref32'] - p64)
    assert np.allclose([de.max(), de.mean(), dp.max(), dp.mean()], s, rtol=1e-12, atol=0)
    # the reference's own output is text with three decimals
    assert np.abs(g['sym/energy_ref3'] - e64).max() <= 5e-4 + 1e-9 and np.abs(g['sym/pitch_ref3'] - p64).max() <= 5e-4 + 1e-9
    d, n = g['sym/dur_int'], g['sym/in_lens']
    assert d.shape == (3, 37) and n.tolist() == [37, 20, 1]
    assert d[0, 0] == 0 and d[0, 36] == 0 and d[0, 10] == 0 and d[0, 11] == 0 and {1, 70, 300} <= set(d[0].tolist())
    assert d[0].sum() == g['sym/frames_energy'].shape[1] and d[1].sum() < d[0].sum() and d.max() <= 512
    assert ((p64 == 0) & (d > 0)).any()                                          # a symbol with frames, none of them voiced


def test_conditioning_restatement_reproduces_the_golden_within_its_spread(g):
    rows = ph.stats_rows(g)
    lens = g['cond/in_lens']
    assert g['cond/energy'].shape == (4, 70) and lens.tolist() == [70, 64, 33, 1]
    valid = np.arange(70)[None, :] < lens[:, None]
    assert 0.15 < (g['cond/energy'][valid] == 0).mean() < 0.35 and 0.15 < (g['cond/pitch'][[0, 1]][valid[[0, 1]]] == 0).mean() < 0.35
    assert not g['cond/pitch'][2].any() and (g['cond/dur_int'][0] == 0).any()
    names = ph.cond_cases(g)
    assert len(names) == 10
    for name in names:
        a = ph.cond_case_args(g, name)
        e64, p64 = ph.condition64(a['energy'], a['pitch'], g['cond/dur_int'], lens, g['cond/energy_factors'], a['pitch_factors'], rows, a['source'],
                                  a['alpha'], a['alpha'], a['mode'], a['normalize'])
        assert np.allclose(e64, g[f'cond/{name}/energy_f64'], rtol=1e-13, atol=1e-15) and np.allclose(p64, g[f'cond/{name}/pitch_f64'], rtol=1e-13, atol=1e-15)
        s = g[f'cond/{name}/spread']
        de, dp = np.abs(g[f'cond/{name}/energy_ref'] - e64), np.abs(g[f'cond/{name}/pitch_ref'] - p64)
        assert np.allclose([de.max(), de.mean(), dp.max(), dp.mean()], s, rtol=1e-9, atol=1e-15), name
        assert s.max() < 1e-5 and not np.isnan(p64).any()
        for b, n in enumerate(lens):                                             # zeros stay zeros, in the reference and in the restatement
            zero_e = (a['energy'][b, :n] == 0) | (g['cond/dur_int'][b, :n] == 0)
            zero_p = (a['pitch'][b, :n] == 0) | (g['cond/dur_int'][b, :n] == 0)
            assert not e64[b, :n][zero_e].any() and not p64[b, :n][zero_p].any() and not e64[b, n:].any() and not p64[b, n:].any()
            assert not g[f'cond/{name}/energy_ref'][b, :n][zero_e].any() and not g[f'cond/{name}/pitch_ref'][b, :n][zero_p].any()


def test_end_to_end_bars_belong_to_the_committed_inference_goldens(g):
    for mode in ('add', 'multiply'):
        case = helpers.load_case(f'inference_{mode}')
        stats = np.array([[0.0, 1.0, *g['e2e/pitch_stats'][i]] for i in case['in/speaker_ids'].tolist()])
        e64, p64 = ph.condition64(case['in/prosody_energy_preds'], case['in/prosody_pitch_preds'], case['out/durations_int'], case['in/input_lengths'],
                                  case['in/energy_factors'], case['in/pitch_factors'], stats, None, 1.0, 1.0, mode, False)
        assert np.allclose(e64, g[f'e2e/inference_{mode}/energy_f64'], rtol=1e-13, atol=1e-15)
        assert np.allclose(p64, g[f'e2e/inference_{mode}/pitch_f64'], rtol=1e-13, atol=1e-15)
        ok_e = ph.within_bar(case['out/energy_preds'], e64, g[f'e2e/inference_{mode}/spread'][:2])
        ok_p = ph.within_bar(case['out/pitch_preds'], p64, g[f'e2e/inference_{mode}/spread'][2:])
        assert ok_e[0] and ok_p[0]


def test_pcm_rule_on_the_edge_values():
    x = np.array([[1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 1.00003, -1.00003, 2.0, -2.0, 0.5 / 32767.5, -0.5 / 32767.5, 0.0, -0.0]], dtype=np.float32)
    assert ph.pcm_rule(x).tolist() == [[32767, -32767, 32767, -32767, 32767, -32768, 32767, -32768, 0, 0, 0, 0]]
    assert ph.pcm_rule(x, [3]).tolist() == [[32767, -32767, 32767] + [0] * 9]


def test_new_launches_are_priced():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[5, 9]])
    assert profiling.price('dx_pcm16', dict(B=2, S=1000), geom) == ('pcm16', 'hbm', None, 2 * 1000 * 6)
    assert profiling.price('dx_symbol_prosody', dict(B=2, T=100, L=10, ldt=100), geom)[0] == 'symbol_prosody'
    assert profiling.price('dx_prosody_condition', dict(B=2, L=10), geom)[3] == 2 * 10 * 32
