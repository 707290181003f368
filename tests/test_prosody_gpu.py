"""The prosody-transfer path on the GPU: symbol means, conditioning and PCM against tests/golden/prosody.npz (float64 restatement, bars
from the reference's own fp32 spread), exact zeros, batch rows bitwise equal to the utterance alone, and ``SpeechSynthesizer`` end to
end against ``GraphedSynthesizer`` + ``infer_batch`` + the numpy PCM rule."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import prosody_helpers as ph
from tests import vocoder_helpers as vh
from ubisoft_laforge_daft_exprt_amd import speech

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
SUM_BOUND = 3.1e-5              # 512 terms x 2^-24: the fp32 summation bound for the longest symbol the fixture may hold


@pytest.fixture(scope='module')
def g():
    return ph.golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- symbol prosody ------------------------------------------------------------------------------------------------------------------
def test_symbol_means_match_float64_and_the_reference_text(g):
    fe, fp, dur, lens = dev(g['sym/frames_energy']), dev(g['sym/frames_pitch']), dev(g['sym/dur_int']), dev(g['sym/in_lens'])
    keep = [t.clone() for t in (fe, fp, dur, lens)]
    se, sp = speech.symbol_prosody(fe, fp, dur, lens)
    assert se.shape == sp.shape == (3, 37) and se.dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip(keep, (fe, fp, dur, lens)))
    for name, got, f64, ref3 in (('energy', se, g['sym/energy_f64'], g['sym/energy_ref3']), ('pitch', sp, g['sym/pitch_f64'], g['sym/pitch_ref3'])):
        got = got.cpu().numpy().astype(np.float64)
        rel = np.abs(got - f64) / np.maximum(np.abs(f64), 1e-30)
        print(f'symbol {name}: max |got - f64| / |f64| {rel[f64 != 0].max():.2e} (bound {SUM_BOUND:.1e}); max |got - text| {np.abs(got - ref3).max():.2e}')
        assert (np.abs(got - f64) <= SUM_BOUND * np.abs(f64)).all(), name
        assert (np.abs(got - ref3) <= 5e-4 + SUM_BOUND * np.abs(ref3)).all(), name
    d, n = g['sym/dur_int'], g['sym/in_lens']
    dead = (d == 0) | (np.arange(37)[None, :] >= n[:, None])
    assert dead[0, 0] and dead[0, 36] and dead[1, 20:].all()
    assert not se.cpu().numpy()[dead].any() and not sp.cpu().numpy()[dead].any()
    assert (se.cpu().numpy()[~dead] > 0).all()
    # each row alone: B = 1, its own symbols, its own frames
    for b in range(3):
        nb = int(n[b])
        tb = int(d[b, :nb].sum())
        e1, p1 = speech.symbol_prosody(fe[b:b + 1, :tb].contiguous(), fp[b:b + 1, :tb].contiguous(), dur[b:b + 1, :nb].contiguous(), lens[b:b + 1])
        assert e1.shape == (1, nb) and torch.equal(e1[0], se[b, :nb]) and torch.equal(p1[0], sp[b, :nb]), b
    # int32 durations and host lengths: same result
    e2, p2 = speech.symbol_prosody(fe, fp, dur.to(torch.int32), n.tolist())
    assert torch.equal(e2, se) and torch.equal(p2, sp)


def test_symbol_durations_past_the_frames_raise_before_launch(g):
    fe, fp = dev(g['sym/frames_energy']), dev(g['sym/frames_pitch'])
    dur = g['sym/dur_int'].copy()
    dur[0, 5] += 1                                           # row 0 used every frame
    with pytest.raises(ValueError, match='row 0'):
        speech.symbol_prosody(fe, fp, dev(dur), dev(g['sym/in_lens']))
    dur[0, 5] -= 1
    dur[1, 25] = 10 ** 6                                     # past row 1's input length: not counted
    speech.symbol_prosody(fe, fp, dev(dur), dev(g['sym/in_lens']))


# ---- conditioning --------------------------------------------------------------------------------------------------------------------
CASES = [f'src{s}_a{a}_{m}' for s in (0, 1) for a in (1.0, 1.3) for m in ('add', 'multiply')] + ['inference_add', 'inference_multiply']


def _run_condition(g, name, rows=slice(None), L=None):
    a = ph.cond_case_args(g, name)
    hp = helpers.golden_hparams(stats=ph.stats_dict(g))
    stats = speech.speaker_stats_table(g['cond/speaker_ids'][rows].tolist(), hp)
    source = None if a['source'] is None else speech.source_stats_row(ph.source_dict(g))
    cut = lambda x: dev(x[rows][:, :L])
    ins = [cut(a['energy']), cut(a['pitch']), cut(g['cond/dur_int']), dev(g['cond/in_lens'][rows].astype(np.int32)), cut(g['cond/energy_factors']),
           cut(a['pitch_factors'])]
    keep = [t.clone() for t in ins]
    e, p = speech._condition(*ins, stats, source, a['alpha'], a['alpha'], ph.MODES[a['mode']], int(a['normalize']))
    assert all(torch.equal(x, y) for x, y in zip(keep, ins)), 'an input was modified'
    return e, p


@pytest.mark.parametrize('name', CASES)
def test_conditioning_matches_float64_within_the_reference_spread(g, name):
    assert name in ph.cond_cases(g)
    e, p = _run_condition(g, name)
    a = ph.cond_case_args(g, name)
    lens, dur = g['cond/in_lens'], g['cond/dur_int']
    s = g[f'cond/{name}/spread']
    en, pn = e.cpu().numpy(), p.cpu().numpy()
    assert not np.isnan(en).any() and not np.isnan(pn).any()
    ok_e, emax, emean = ph.within_bar(en, g[f'cond/{name}/energy_f64'], s[:2])
    ok_p, pmax, pmean = ph.within_bar(pn, g[f'cond/{name}/pitch_f64'], s[2:])
    print(f'{name}: energy max {emax:.2e} (ref {s[0]:.2e}) mean {emean:.2e} (ref {s[1]:.2e}); pitch max {pmax:.2e} (ref {s[2]:.2e}) mean {pmean:.2e} (ref {s[3]:.2e})')
    assert ok_e and ok_p, (name, emax, emean, pmax, pmean, s)
    pad = np.arange(70)[None, :] >= lens[:, None]
    assert not en[pad].any() and not pn[pad].any()
    assert not en[(a['energy'] == 0) | (dur == 0)].any() and not pn[(a['pitch'] == 0) | (dur == 0)].any()
    assert not pn[2].any() and (pn[0] != 0).any()                             # the all-unvoiced row; a voiced one
    for b, n in enumerate(lens.tolist()):                                     # the utterance alone: B = 1, L = its own length
        e1, p1 = _run_condition(g, name, rows=slice(b, b + 1), L=n)
        assert torch.equal(e1[0], e[b, :n]) and torch.equal(p1[0], p[b, :n]), (name, b)


def test_condition_external_prosody_covers_the_reference_call(g):
    """generate.py:213-278 as one call: durations exactly the reference's, energy / pitch the kernel's normalisation (no factors, no
    transform), from entries and from padded tensors alike."""
    hp = helpers.golden_hparams(stats=ph.stats_dict(g))
    lens = g['cond/in_lens'].tolist()
    entries = [{'symbols': ['a'] * n, 'durations_frames': g['cond/durations_frames'][b, :n].tolist(), 'energy': g['cond/energy'][b, :n].tolist(),
                'pitch': g['cond/pitch'][b, :n].tolist()} for b, n in enumerate(lens)]
    tensors = {'durations_frames': torch.from_numpy(g['cond/durations_frames']), 'energy': dev(g['cond/energy']), 'pitch': dev(g['cond/pitch']),
               'input_lengths': torch.tensor(lens)}
    ids = g['cond/speaker_ids'].tolist()
    out = speech.condition_external_prosody(entries, ids, hp, alpha_dur=1.3, device=DEV)
    out_t = speech.condition_external_prosody(tensors, torch.tensor(ids), hp, alpha_dur=1.3, device=DEV)
    assert set(out) == {'duration_preds', 'durations_int', 'energy_preds', 'pitch_preds'}
    for k in out:
        assert out[k].device.type == 'cuda' and torch.equal(out[k], out_t[k]), k
    assert np.array_equal(out['duration_preds'].cpu().numpy(), g['dur/a1.3/seconds']) and np.array_equal(out['durations_int'].cpu().numpy(), g['dur/a1.3/int'])
    # the reference's own normalised values (alpha 1, no source): its error against float64 sets the bar
    e64, p64 = ph.condition64(g['cond/energy'], g['cond/pitch'], None, lens, None, None, ph.stats_rows(g), None, 1.0, 1.0, 'none', True)
    for got, ref, f64 in ((out['energy_preds'], g['cond/norm_energy'], e64), (out['pitch_preds'], g['cond/norm_pitch'], p64)):
        d = np.abs(ref - f64)
        ok, dmax, dmean = ph.within_bar(got.cpu().numpy(), f64, (d.max(), d.mean()))
        print(f'normalisation: max {dmax:.2e} (ref {d.max():.2e}) mean {dmean:.2e} (ref {d.mean():.2e})')
        assert ok
        assert not got.cpu().numpy()[ref == 0].any()


# ---- PCM -----------------------------------------------------------------------------------------------------------------------------
def test_pcm_is_the_numpy_rule_bitwise():
    B, S, lengths = 3, 1031, [1031, 1024, 5]
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((B, S)) * 0.6).astype(np.float32)
    edge = np.array([1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 1.00003, -1.00003, 2.0, -2.0, 0.5 / 32767.5, -0.5 / 32767.5, 0.0, -0.0], dtype=np.float32)
    x[0, :12], x[0, -12:], x[1, 1012:1024], x[2, :5] = edge, edge, edge, edge[[0, 1, 5, 9, 11]]
    x[2, 5:] = 0.7                                           # past the row's length: must come out as 0
    want = ph.pcm_rule(x, lengths)
    xd = dev(x)
    got = speech.to_pcm16(xd, lengths)
    assert got.dtype == torch.int16 and got.shape == (B, S) and torch.equal(xd, dev(x))
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(speech.to_pcm16(xd, torch.tensor(lengths, device=DEV)).cpu().numpy(), want)
    for b, n in enumerate(lengths):
        assert not got[b, n:].any()
    for s in (1, 7, 8, 9, 17):                               # rows shorter than, equal to and just past one vector
        assert np.array_equal(speech.to_pcm16(dev(x[:, :s]), [s, s, min(s, 5)]).cpu().numpy(), ph.pcm_rule(np.ascontiguousarray(x[:, :s]), [s, s, min(s, 5)]))


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
E2E_STATS = {'spk 0': {'energy': {'mean': 2.0, 'std': 1.5}, 'pitch': {'mean': 5.0, 'std': 0.25}},
             'spk 1': {'energy': {'mean': 1.7, 'std': 1.1}, 'pitch': {'mean': 4.6, 'std': 0.3}}}


@pytest.fixture(scope='module')
def parts(g):
    import ubisoft_laforge_daft_exprt_amd as dx
    from ubisoft_laforge_daft_exprt_amd import vocoder as voc
    assert np.array_equal(g['e2e/pitch_stats'], [[5.0, 0.25], [4.6, 0.3]])
    dx.set_precision('f32')
    hp = helpers.golden_hparams(stats=E2E_STATS)
    model = dx.DaftExprt(hp).to(DEV)
    model.load_state_dict(helpers.golden_state_dict(), strict=True)
    return dx, hp, model.eval(), voc.HiFiGanVocoder(vh.state_dict(), device=DEV, precision='f32')


def _case_args(case, dur_scale=1.0, emb=lambda t: t):
    t = lambda k: torch.from_numpy(case[k]).clone().to(DEV)
    inputs = (t('in/symbols'), t('in/dur_factors') * dur_scale, t('in/energy_factors'), t('in/pitch_factors'), t('in/input_lengths'), t('in/speaker_ids'))
    prosody = {k: t('in/prosody_' + k) for k in ('duration_preds', 'durations_int', 'energy_preds', 'pitch_preds')}
    return inputs, prosody, emb(t('in/spk_embs')), t('in/accent_emb')


def _check_call(g, parts, synth, plain, case, transform, use_graph, dur_scale, emb, stored):
    dx, hp, model, vocoder = parts
    inputs, prosody, embs, accent = _case_args(case, dur_scale, emb)
    keep = {k: v.clone() for k, v in prosody.items()}
    out = synth(inputs, transform, prosody, embs, accent, use_graph=use_graph)
    assert set(out) == {'pcm', 'audio', 'sample_lengths', 'mel', 'output_lengths', 'encoder_preds', 'weights'}
    assert all(torch.equal(prosody[k], keep[k]) for k in keep)
    dur, dur_int, energy, pitch, in_lens = out['encoder_preds']
    # the same forward through GraphedSynthesizer, given the conditioning kernel's own output and factors that change nothing
    inputs2, _, embs2, accent2 = _case_args(case, dur_scale, emb)
    neutral = (inputs2[0], inputs2[1], torch.ones_like(inputs2[2]), torch.zeros_like(inputs2[3]), inputs2[4], inputs2[5])
    fed = {'duration_preds': keep['duration_preds'].clone(), 'durations_int': keep['durations_int'].clone(), 'energy_preds': energy.clone(),
           'pitch_preds': pitch.clone()}
    enc2, (mel2, lens2), w2 = plain(neutral, 'multiply', fed, embs2, accent2, use_graph=use_graph)
    assert torch.equal(enc2[1], dur_int) and torch.equal(enc2[0], dur) and torch.equal(enc2[2], energy) and torch.equal(enc2[3], pitch)
    assert torch.equal(out['mel'], mel2) and torch.equal(out['output_lengths'], lens2) and torch.equal(out['weights'], w2)
    audio2, slen2 = vocoder.infer_batch(mel2, lens2)
    assert torch.equal(out['audio'], audio2) and torch.equal(out['sample_lengths'], slen2)
    assert out['pcm'].dtype == torch.int16 and out['pcm'].device.type == 'cuda'
    assert np.array_equal(out['pcm'].cpu().numpy(), ph.pcm_rule(audio2.cpu().numpy(), slen2.tolist()))
    assert out['pcm'].abs().max().item() > 0
    # energy / pitch predictions: the float64 restatement on this call's integer durations, the bar from the stored golden's own spread
    s = g[f'e2e/inference_{transform}/spread']
    stats = np.array([[0.0, 1.0, *g['e2e/pitch_stats'][i]] for i in case['in/speaker_ids'].tolist()])
    e64, p64 = ph.condition64(case['in/prosody_energy_preds'], case['in/prosody_pitch_preds'], dur_int.cpu().numpy(), case['in/input_lengths'],
                              case['in/energy_factors'], case['in/pitch_factors'], stats, None, 1.0, 1.0, transform, False)
    for name, got, f64, sp, key in (('energy', energy, e64, s[:2], 'out/energy_preds'), ('pitch', pitch, p64, s[2:], 'out/pitch_preds')):
        ok, dmax, dmean = ph.within_bar(got.cpu().numpy(), f64, sp)
        print(f'{transform} graph={use_graph} x{dur_scale} {name}: vs f64 max {dmax:.2e} mean {dmean:.2e} (stored golden {sp[0]:.2e} / {sp[1]:.2e})')
        assert ok, (name, dmax, dmean, sp)
        if stored:
            ok, dmax, dmean = ph.within_bar(got.cpu().numpy(), case[key].astype(np.float64), sp)
            assert ok, (name, 'stored', dmax, dmean, sp)
    if stored:
        assert np.array_equal(dur_int.cpu().numpy(), case['out/durations_int']) and np.array_equal(out['output_lengths'].cpu().numpy(), case['out/output_lengths'])
        assert np.array_equal(e64, g[f'e2e/inference_{transform}/energy_f64']) and np.array_equal(p64, g[f'e2e/inference_{transform}/pitch_f64'])
    return out


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('transform', ['add', 'multiply'])
def test_speech_synthesizer_end_to_end(g, parts, transform, use_graph):
    from ubisoft_laforge_daft_exprt_amd.inference import GraphedSynthesizer
    dx, hp, model, vocoder = parts
    case = helpers.load_case(f'inference_{transform}')
    synth = dx.SpeechSynthesizer(model, hp, vocoder)
    plain = GraphedSynthesizer(model, hp)
    first = _check_call(g, parts, synth, plain, case, transform, use_graph, 1.0, lambda t: t, stored=True)
    # another batch of the same (L up to 16, T up to 64) bucket: other durations, other speaker embeddings
    second = _check_call(g, parts, synth, plain, case, transform, use_graph, 0.93, lambda t: t * 0.5 + 0.1, stored=False)
    assert second['mel'].shape[2] != first['mel'].shape[2] and second['mel'].shape[2] <= 64
    assert len(synth.synth.graphs) == (1 if use_graph else 0)
    if use_graph:
        assert next(iter(synth.synth.graphs.values())).hits == 2
    a = _case_args(case)
    without = synth(a[0], transform, a[1], a[2], a[3], pcm16=False, use_graph=use_graph)
    assert without['pcm'] is None and torch.equal(without['audio'], first['audio'])
    with pytest.raises(ValueError, match='raw reference prosody'):
        synth(a[0], transform, a[1], a[2], a[3], alpha_pitch=1.3)


def test_raw_reference_prosody_and_reference_audio(g, parts):
    """Raw prosody goes through the same single launch with the normalisation switched on; ``from_reference_audio`` is the mel front end,
    ``symbol_prosody`` and that call."""
    from ubisoft_laforge_daft_exprt_amd import mel as melmod
    dx, hp, model, vocoder = parts
    case = helpers.load_case('inference_add')
    synth = dx.SpeechSynthesizer(model, hp, vocoder)
    inputs, _, embs, accent = _case_args(case)
    lens = case['in/input_lengths'].tolist()
    rng = np.random.default_rng(17)
    wav_lens = [16000, 12000, 9000]                          # 62, 46, 35 frames
    wavs = dev((0.3 * rng.standard_normal((3, 16000))).astype(np.float32))
    dur = np.zeros((3, 10), dtype=np.int64)
    for b, n in enumerate(lens):
        dur[b, :n] = rng.integers(0, 5, n)
    frames_pitch = (5.0 + 0.3 * rng.standard_normal((3, 70))).astype(np.float32)
    frames_pitch[rng.random((3, 70)) < 0.3] = 0.0
    source = ph.source_dict(g)
    kw = dict(source_stats=source, alpha_dur=1.2, alpha_pitch=1.3, alpha_energy=0.8, use_graph=False)
    out = synth.from_reference_audio(wavs, wav_lens, dev(frames_pitch), torch.from_numpy(dur), inputs, 'add', embs, accent, **kw)
    # by hand
    _, energy, _ = melmod.MelSpectrogram(hp, device=DEV)(wavs, wav_lens)
    T = energy.shape[1]
    se, sp = speech.symbol_prosody(energy, dev(frames_pitch)[:, :T].contiguous(), dev(dur), inputs[4])
    raw = {'durations_frames': torch.from_numpy(dur).float(), 'energy': se, 'pitch': sp, 'input_lengths': inputs[4]}
    by_hand = synth(inputs, 'add', raw, embs, accent, **kw)
    for k in ('pcm', 'audio', 'mel', 'weights', 'output_lengths'):
        assert torch.equal(out[k], by_hand[k]), k
    # the conditioning stage of that call, launched directly
    secs = torch.zeros(3, 10)
    for b, n in enumerate(lens):
        secs[b, :n] = speech.host_durations(dur[b, :n].astype(np.float32), 1.2, hp)[0]
    from ubisoft_laforge_daft_exprt_amd.durations import get_int_durations
    d_f, d_i = get_int_durations(secs.to(DEV) * inputs[1], hp)
    e, p = speech._condition(se, sp, d_i, inputs[4].to(torch.int32), inputs[2], inputs[3], speech.speaker_stats_table(inputs[5], hp),
                             speech.source_stats_row(source), 0.8, 1.3, 1, 1)
    enc = out['encoder_preds']
    assert torch.equal(enc[0], d_f) and torch.equal(enc[1], d_i) and torch.equal(enc[2], e) and torch.equal(enc[3], p)
    e64, p64 = ph.condition64(se.cpu().numpy(), sp.cpu().numpy(), d_i.cpu().numpy(), lens, case['in/energy_factors'], case['in/pitch_factors'],
                              np.array([[2.0, 1.5, 5.0, 0.25], [1.7, 1.1, 4.6, 0.3]])[case['in/speaker_ids']], g['cond/source_stats'].astype(np.float64),
                              0.8, 1.3, 'add', True)
    assert not torch.isnan(e).any() and not torch.isnan(p).any() and (p != 0).any()
    # no fixture holds a spread for these inputs, so the bound is the arithmetic's own: at most 8 fp32 roundings of half an ulp of the largest
    # magnitude in the chain, amplified by 1 / std <= 4 and alpha <= 1.3 (21 ulp, taken as 64); the add transform itself runs in double
    for got, f64, x in ((e, e64, se), (p, p64, sp)):
        scale = max(1.0, float(x.abs().max()), float(np.abs(f64).max()))
        assert np.abs(got.cpu().numpy() - f64).max() <= 64 * 2.0 ** -24 * scale
