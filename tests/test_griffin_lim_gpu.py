"""Griffin-Lim on the GPU: the iteration against the reference signals of tests/golden/griffin_lim.npz and the float64 restatement
(bars from the float32 spread of the same steps, the rule of tests/test_mel_gpu.py), tile edges, batch rows bitwise equal to the
utterance alone, graph replay, convergence, the NNLS residual against the reference's, the composition of ``from_mel`` and
``SpeechSynthesizer`` with a ``GriffinLimVocoder``."""
import numpy as np
import pytest
import torch

from tests import griffin_lim_helpers as gh
from tests import helpers
from ubisoft_laforge_daft_exprt_amd import griffin_lim as gl
from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return gh.golden()


@pytest.fixture(scope='module')
def engine():
    return gl.GriffinLim(device=DEV)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bar(name, got, x64, spread_max):
    d = np.abs(got.astype(np.float64) - x64).max()
    bar = 4 * spread_max + 1e-6 * np.abs(x64).max()
    print(f'{name}: max |device - f64| {d:.3e}, float32 spread {spread_max:.3e}, bar {bar:.3e} (ratio to the spread {d / max(spread_max, 1e-300):.2f})')
    return d, bar


@pytest.mark.parametrize('start_name', gh.STARTS)
def test_parity_with_the_reference_signals(g, engine, start_name):
    M = dev(g['speech/nnls'][:, :-2])[None]
    T = M.shape[2]
    S = 256 * T + 1024
    start = dev(g['noise'] if start_name == 'noise' else np.zeros(S, dtype=np.float32))[None]
    fails = []
    for k in gh.ITERS:
        x, lens = engine.reconstruct(M, [T], init=start, iterations=k, use_graph=False)
        assert x.shape == (1, S) and lens.tolist() == [S]
        d, bar = _bar(f'{start_name} {k}', x[0].cpu().numpy(), g[f'gl/{start_name}/{k}'], g[f'gl/{start_name}/{k}/spread'][0])
        if not d <= bar:
            fails.append((k, d, bar))
        assert not x[0, 256 * T + 768:].any()
    assert not fails, fails


def _tile():
    return gl.layout()[0]


def _edge_frames():
    own = _tile()
    return sorted({1, 2, 3, 4, own - 1, own, own + 1, 2 * own + 3} | {max(1, n - 3) for n in (own - 1, own, own + 1, 2 * own + 3)})


def test_tile_edges_against_the_float64_restatement(engine):
    """Rows shorter than the overlap (1 .. 4 frames) and rows whose frame count, or whose count of signal-carrying hop blocks
    (frames + 3), sits at the tile's own block count - 1, + 0, + 1 and at twice it + 3."""
    rng = np.random.default_rng(5)
    fails = []
    for T in _edge_frames():
        M = (np.abs(rng.standard_normal((513, T))) * np.exp(-np.arange(513) / 120.0)[:, None]).astype(np.float32)
        x0 = rng.standard_normal(256 * T + 1024).astype(np.float32)
        x64 = gh.gl_iterate(M.astype(np.float64), x0, 8, np.float64)
        x32 = gh.gl_iterate(M, x0, 8, np.float32)
        x, lens = engine.reconstruct(dev(M)[None], [T], init=dev(x0)[None], iterations=8, use_graph=False)
        assert lens.tolist() == [256 * T + 1024]
        d, bar = _bar(f'T {T}', x[0].cpu().numpy(), x64, np.abs(x32.astype(np.float64) - x64).max())
        if not d <= bar:
            fails.append((T, d, bar))
    assert not fails, fails


BATCH = [29, 1, 14, 10, 4, 0]


def _batch(g):
    own = _tile()
    frames = BATCH[:2] + [own + 1, own - 3] + BATCH[4:]
    T = max(frames)
    rng = np.random.default_rng(9)
    M = np.full((len(frames), 513, T), 1e3, dtype=np.float32)          # past a row's frames / samples: garbage that must never be read
    x0 = np.full((len(frames), 256 * T + 1024), 1e3, dtype=np.float32)
    src = g['speech/nnls']
    for b, n in enumerate(frames):
        M[b, :, :n] = src[:, (b + np.arange(n)) % src.shape[1]]
        x0[b, :256 * n + 1024] = rng.standard_normal(256 * n + 1024)
    return frames, dev(M), dev(x0)


def test_batch_rows_equal_utterances_alone_bitwise(g, engine):
    frames, M, x0 = _batch(g)
    c0 = engine.captures
    keep_M, keep_x0 = M.clone(), x0.clone()
    x, lens = engine.reconstruct(M, frames, init=x0, iterations=6, use_graph=False)
    assert torch.equal(M, keep_M) and torch.equal(x0, keep_x0)
    assert lens.tolist() == [256 * n + 1024 if n else 0 for n in frames] and torch.isfinite(x).all()
    for b, n in enumerate(frames):
        assert torch.count_nonzero(x[b, int(lens[b]):]).item() == 0
        if n == 0:
            continue
        alone, alone_len = engine.reconstruct(M[b:b + 1, :, :n].contiguous(), [n], init=x0[b:b + 1, :256 * n + 1024].contiguous(), iterations=6,
                                              use_graph=False)
        assert alone_len.tolist() == [256 * n + 1024]
        assert torch.equal(x[b, :256 * n + 1024], alone[0]), (b, n)
        assert x[b].abs().max().item() > 0
    again, _ = engine.reconstruct(M, torch.tensor(frames, device=DEV), init=x0, iterations=6, use_graph=False)
    assert torch.equal(x, again)
    for _ in range(2):                                                 # capture, then a replay of the cached graph
        graphed, glens = engine.reconstruct(M, frames, init=x0, iterations=6, use_graph=True)
        assert torch.equal(x, graphed) and torch.equal(lens, glens)
    assert engine.captures == c0 + 1
    x1 = torch.randn(x0.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    other, _ = engine.reconstruct(M, frames, init=x1, iterations=6, use_graph=True)           # same graph, other contents
    eager, _ = engine.reconstruct(M, frames, init=x1, iterations=6, use_graph=False)
    assert torch.equal(other, eager) and engine.captures == c0 + 1 and not torch.equal(other, x)


def test_convergence_matches_the_reference(g, engine):
    M = g['speech/nnls'][:, :-2]
    T = M.shape[1]
    x, _ = engine.reconstruct(dev(M)[None], [T], init=dev(g['noise'])[None], iterations=128, use_graph=True)
    sc, ref = gh.spectral_convergence(x[0].cpu().numpy().astype(np.float64), M), float(g['gl/convergence'])
    print(f'spectral convergence after 128 iterations: device {sc:.6e}, reference {ref:.6e} (relative deviation {abs(sc - ref) / ref:.2e})')
    assert abs(sc - ref) <= 1e-3 * ref


def test_nnls_reaches_the_reference_residual(g, engine):
    A = mel_filter_bank(22050, 1024, 80, 0.0, 8000.0)
    names = ('speech', 'chirp')
    lin = [np.exp(g[f'{n}/mel']) for n in names]
    lens = [m.shape[1] for m in lin]
    T = max(lens)
    batch = np.full((2, 80, T), 1e3, dtype=np.float32)                 # past a row's frames: garbage that must never show
    for b, m in enumerate(lin):
        batch[b, :, :lens[b]] = m
    X = engine.mel_to_linear(dev(batch), lens)
    assert X.shape == (2, 513, T) and X.dtype == torch.float32
    assert (X >= 0).all() and torch.isfinite(X).all()
    for b, name in enumerate(names):
        res, ref = gh.relative_residual(A, X[b, :, :lens[b]].cpu().numpy(), lin[b]), float(g[f'{name}/residual'])
        print(f'{name}: device NNLS residual {res:.3e}, reference {ref:.3e}')
        assert res <= ref, (name, res, ref)
        assert torch.count_nonzero(X[b, :, lens[b]:]).item() == 0
        alone = engine.mel_to_linear(dev(lin[b])[None], [lens[b]])
        assert torch.equal(alone[0], X[b, :, :lens[b]]), name
    assert torch.equal(engine.mel_to_linear(dev(batch), torch.tensor(lens, device=DEV)), X)


def test_from_mel_is_the_composition(g, engine):
    mel = g['speech/mel']
    lens = [40, 2, 17, 3]
    T = max(lens)
    mels = np.full((len(lens), 80, T), -3.0, dtype=np.float32)
    for b, n in enumerate(lens):
        mels[b, :, :n] = mel[:, b:b + n]
    mels = dev(mels)
    init = torch.randn(len(lens), 256 * (T - 2) + 1024, generator=torch.Generator().manual_seed(4)).to(DEV)
    audio, slen = engine.from_mel(mels, lens, init=init, iterations=8)
    assert audio.shape == (len(lens), 256 * T + 512)
    assert slen.tolist() == [256 * n + 512 if n >= 3 else 0 for n in lens]
    X = engine.mel_to_linear(torch.exp(mels), lens)
    x, xlen = engine.reconstruct(X[:, :, :T - 2], [max(n - 2, 0) for n in lens], init=init, iterations=8)
    assert torch.equal(audio, engine.peak_normalize(x)) and torch.equal(slen, xlen)
    for b, n in enumerate(lens):
        assert torch.count_nonzero(audio[b, int(slen[b]):]).item() == 0
        if n < 3:
            assert not audio[b].any()                                  # the reference raises on such a row; here it is silent
            continue
        assert audio[b].abs().max().item() == 1.0
        alone, alen = engine.from_mel(mels[b:b + 1, :, :n].contiguous(), [n], init=init[b:b + 1, :256 * (n - 2) + 1024].contiguous(), iterations=8)
        assert alen.tolist() == [256 * n + 512] and torch.equal(alone[0], audio[b, :256 * n + 512]), (b, n)
    # an all-zero signal stays zero under the peak normalisation (the reference would produce NaN)
    z = engine.peak_normalize(torch.zeros(2, 1000, device=DEV))
    assert not z.any() and torch.isfinite(z).all()
    # the numpy drop-in is row 0 of the batched call
    hp = type('HP', (), dict(sampling_rate=22050, filter_length=1024, hop_length=256, n_mel_channels=80, mel_fmin=0.0, mel_fmax=8000.0))()
    got = gl.griffin_lim_reconstruction_from_mel_spec(mel[:, :40], hp, None, iterations=8, init=init[0].cpu().numpy(), device=DEV)
    assert isinstance(got, np.ndarray) and got.shape == (256 * 40 + 512,)
    assert np.array_equal(got, audio[0].cpu().numpy())
    with pytest.raises(NotImplementedError):
        gl.griffin_lim_reconstruction_from_mel_spec(mel, type('HP', (), dict(hop_length=128))(), None)


E2E_STATS = {'spk 0': {'energy': {'mean': 2.0, 'std': 1.5}, 'pitch': {'mean': 5.0, 'std': 0.25}},
             'spk 1': {'energy': {'mean': 1.7, 'std': 1.1}, 'pitch': {'mean': 4.6, 'std': 0.3}}}


def _case_args(case):
    t = lambda k: torch.from_numpy(case[k]).clone().to(DEV)
    inputs = (t('in/symbols'), t('in/dur_factors'), t('in/energy_factors'), t('in/pitch_factors'), t('in/input_lengths'), t('in/speaker_ids'))
    prosody = {k: t('in/prosody_' + k) for k in ('duration_preds', 'durations_int', 'energy_preds', 'pitch_preds')}
    return inputs, prosody, t('in/spk_embs'), t('in/accent_emb')


def test_speech_synthesizer_with_griffin_lim_and_unchanged_with_hifigan():
    import ubisoft_laforge_daft_exprt_amd as dx
    from tests import vocoder_helpers as vh
    from ubisoft_laforge_daft_exprt_amd import speech
    dx.set_precision('f32')
    hp = helpers.golden_hparams(stats=E2E_STATS)
    model = dx.DaftExprt(hp).to(DEV)
    model.load_state_dict(helpers.golden_state_dict(), strict=True)
    model.eval()
    case = helpers.load_case('inference_add')
    gen = torch.Generator(device=DEV).manual_seed(21)
    synth = dx.SpeechSynthesizer(model, hp, dx.GriffinLimVocoder(hp, iterations=8, device=DEV, generator=gen))
    a = _case_args(case)
    out = synth(a[0], 'add', a[1], a[2], a[3])
    T = out['mel'].shape[2]
    frames = out['output_lengths'].tolist()
    assert out['audio'].shape == (len(frames), 256 * T + 512) and out['audio'].dtype == torch.float32
    assert out['sample_lengths'].tolist() == [256 * n + 512 for n in frames] and min(frames) >= 3
    assert out['pcm'].dtype == torch.int16 and torch.equal(out['pcm'], speech.to_pcm16(out['audio'], out['sample_lengths']))
    assert out['pcm'].abs().max().item() == 32767
    for b, n in enumerate(out['sample_lengths'].tolist()):
        assert not out['audio'][b, n:].any() and not out['pcm'][b, n:].any()
    with pytest.raises(NotImplementedError, match='causal'):
        synth.stream(a[0], 'add', a[1], a[2], a[3])
    one = synth.vocoder.infer(out['mel'][0, :, :frames[0]])               # the reference vocoder's one-utterance contract
    assert isinstance(one, np.ndarray) and one.shape == (256 * frames[0] + 512,) and np.abs(one).max() == 1.0
    # the HiFi-GAN path is untouched: the same call against the vocoder and the PCM rule applied by hand
    vocoder = dx.HiFiGanVocoder(vh.state_dict(), device=DEV, precision='f32')
    hifi = dx.SpeechSynthesizer(model, hp, vocoder)
    b = _case_args(case)
    got = hifi(b[0], 'add', b[1], b[2], b[3])
    assert torch.equal(got['mel'], out['mel']) and torch.equal(got['output_lengths'], out['output_lengths'])
    audio, slen = vocoder.infer_batch(got['mel'], got['output_lengths'])
    assert torch.equal(got['audio'], audio) and torch.equal(got['sample_lengths'], slen) and torch.equal(slen, got['output_lengths'] * 256)
    assert torch.equal(got['pcm'], speech.to_pcm16(audio, slen))
    assert len(hifi.stream(b[0], 'add', b[1], b[2], b[3])['chunks']) >= 1
