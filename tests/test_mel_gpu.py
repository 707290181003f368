"""The gfx950 mel front end on the GPU: parity with the reference golden (fp64 restatement, bars set by the reference's own fp32
spread), zeros and frame counts, batch rows bitwise equal to the utterance alone, graph replay, the reference-signature drop-ins,
and the accent embedding from audio."""
import numpy as np
import pytest
import torch

from tests import helpers
from tests import mel_helpers as mh
from ubisoft_laforge_daft_exprt_amd import mel

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return mh.golden()


@pytest.fixture(scope='module')
def frontends():
    return {v: mel.MelSpectrogram(fmax=fmax, device=DEV) for v, fmax in mh.FMAX.items()}


def _check(name, v, got_mel, got_energy, e):
    dm, de = np.abs(got_mel.astype(np.float64) - e['f64']), np.abs(got_energy.astype(np.float64) - e['energy_f64'])
    s = e['spread']
    print(f'{name:12s} {v}: mel max {dm.max():.2e} (ref {s[0]:.2e}) mean {dm.mean():.2e} (ref {s[1]:.2e}); '
          f'energy max {de.max():.2e} (ref {s[2]:.2e}) mean {de.mean():.2e} (ref {s[3]:.2e})')
    assert dm.max() <= 4 * s[0] + 1e-6 and dm.mean() <= 2 * s[1] + 1e-7, (name, v, dm.max(), dm.mean(), s)
    assert de.max() <= 4 * s[2] + 1e-6 and de.mean() <= 2 * s[3] + 1e-7, (name, v, de.max(), de.mean(), s)


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_parity_with_reference_golden(golden, frontends, v):
    for name, d in golden.items():
        w = torch.from_numpy(d['wav'])[None].to(DEV)
        mels, energy, frames = frontends[v](w, [w.shape[1]])
        T = w.shape[1] // 256
        assert mels.shape == (1, 80, T) and energy.shape == (1, T) and frames.tolist() == [T]
        _check(name, v, mels[0].cpu().numpy(), energy[0].cpu().numpy(), d[v])


BATCH = [33054, 20000, 1000, 513, 512, 511, 385]


def _batch(golden):
    speech = torch.from_numpy(golden['speech']['wav'])
    g = torch.Generator().manual_seed(11)
    S = max(BATCH)
    wavs = torch.full((len(BATCH), S), 1e3)                           # past each row's length: garbage that must never be read
    for b, n in enumerate(BATCH):
        wavs[b, :n] = speech[:n] if b % 2 == 0 else 0.3 * torch.randn(n, generator=g)
    return wavs.to(DEV)


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_batch_rows_equal_utterances_alone_bitwise(golden, frontends, v):
    fe = frontends[v]
    wavs = _batch(golden)
    mels, energy, frames = fe(wavs, BATCH)
    T = max(BATCH) // 256
    assert mels.shape == (len(BATCH), 80, T) and energy.shape == (len(BATCH), T)
    assert frames.tolist() == [n // 256 for n in BATCH]
    for b, n in enumerate(BATCH):
        t = n // 256
        assert torch.count_nonzero(mels[b, :, t:]).item() == 0 and torch.count_nonzero(energy[b, t:]).item() == 0
        alone_m, alone_e, alone_f = fe(wavs[b:b + 1, :n].contiguous(), [n])
        assert alone_m.shape == (1, 80, t) and alone_f.tolist() == [t]
        assert torch.equal(mels[b, :, :t], alone_m[0]) and torch.equal(energy[b, :t], alone_e[0]), (v, b, n)
        assert torch.isfinite(alone_m).all() and (alone_e > 0).all()
    # lengths as a device tensor: same result
    m2, e2, f2 = fe(wavs, torch.tensor(BATCH, device=DEV))
    assert torch.equal(mels, m2) and torch.equal(energy, e2) and torch.equal(frames, f2)


def test_bad_lengths_raise_before_launch(frontends):
    w = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(ValueError):
        frontends['hifi'](w, [1000, 384])
    with pytest.raises(ValueError):
        frontends['hifi'](w, torch.tensor([1001, 500], device=DEV))


def test_graph_replay_equals_eager_bitwise(golden, frontends):
    fe = frontends['hifi']
    static = _batch(golden)
    fe(static, BATCH)                                                # eager warm-up: packs the basis, caches the lengths
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        outs = fe(static, BATCH)
    g = torch.Generator().manual_seed(3)
    for _ in range(2):
        new = (0.2 * torch.randn(static.shape, generator=g)).to(DEV)
        static.copy_(new)
        graph.replay()
        ref = fe(new, BATCH)
        for a, b in zip(outs, ref):
            assert torch.equal(a, b)


def test_drop_ins_match_golden(golden):
    hp = type('HP', (), dict(mel_fmin=0.0, mel_fmax=8000.0, hop_length=256, filter_length=1024, n_mel_channels=80,
                             sampling_rate=22050, min_clipping=1e-5))()
    for name, d in golden.items():
        got = mel.mel_spectrogram_HiFi(d['wav'], hp)
        assert isinstance(got, np.ndarray) and got.shape == d['hifi']['f64'].shape
        dm = np.abs(got - d['hifi']['f64'])
        assert dm.max() <= 4 * d['hifi']['spread'][0] + 1e-6, name
    names = ['speech', 'edge513']
    n = min(len(golden[k]['wav']) for k in names)
    y = torch.stack([torch.from_numpy(golden[k]['wav'][:n]) for k in names]).to(DEV)
    got = mel.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, None, center=False)
    assert got.shape == (2, 80, n // 256) and got.device == y.device
    ref = mel.MelSpectrogram(fmax=None, device=DEV)(y, [n, n])[0]
    assert torch.equal(got, ref)
    e = golden['edge513']['full']
    assert np.abs(got[1].cpu().numpy() - e['f64']).max() <= 4 * e['spread'][0] + 1e-6


@pytest.mark.parametrize('use_graph', [False, True])
def test_accent_embeddings_from_audio(golden, use_graph):
    import ubisoft_laforge_daft_exprt_amd as dx
    from ubisoft_laforge_daft_exprt_amd.inference import GraphedSynthesizer
    dx.set_precision('f32')
    hp = helpers.golden_hparams()
    model = dx.DaftExprt(hp).to(DEV)
    model.load_state_dict(helpers.golden_state_dict(), strict=True)
    synth = GraphedSynthesizer(model.eval(), hp)
    wavs = _batch(golden)[:4]
    wav_lens = BATCH[:4]
    frames = [n // 256 for n in wav_lens]                             # 129, 78, 3, 2
    pitch_lens = [120, 90, 2, 2]                                      # shorter, longer, shorter, equal
    g = torch.Generator().manual_seed(9)
    pitch = (torch.randn(4, 130, generator=g) + 5.0).to(DEV)
    got = synth.accent_embeddings_from_audio(wavs, wav_lens, pitch, pitch_lens, use_graph=use_graph)
    assert got.shape == (4, 128)
    # what it must be: MelSpectrogram with the synthesizer's hparams, each row trimmed to min(pitch, mel) frames
    mels, energy, _ = mel.MelSpectrogram(hp, device=DEV)(wavs, wav_lens)
    n = [min(p, f) for p, f in zip(pitch_lens, frames)]
    T = max(n)
    keep = (torch.arange(T)[None, :] < torch.tensor(n)[:, None]).to(DEV)
    e = energy[:, :T].masked_fill(~keep, 0.0).contiguous()
    p = pitch[:, :T].masked_fill(~keep, 0.0).contiguous()
    m = mels[:, :, :T].masked_fill(~keep[:, None, :], 0.0).contiguous()
    want = synth.accent_embeddings(e, p, m, torch.tensor(n, device=DEV), use_graph=use_graph)
    assert torch.equal(got, want)
    mean = synth.accent_embedding_from_audio(wavs, wav_lens, pitch, pitch_lens, use_graph=use_graph)
    assert mean.shape == (1, 128) and torch.equal(mean, want.mean(dim=0, keepdim=True))
