"""CPU checks of the mel front end's host side: the Slaney filter bank (closed-form values; librosa is not installed, so the table is
not compared with librosa itself), frame counts against torch.stft, argument validation before any launch, the profiler's pricing
of dx_mel, and the self-consistency of tests/golden/mel_frontend.npz."""
import numpy as np
import pytest
import torch

from tests import mel_helpers as mh
from ubisoft_laforge_daft_exprt_amd import mel, profiling


def test_slaney_mel_scale_values():
    assert abs(float(mel.hz_to_mel(1000.0)) - 15.0) < 1e-12
    assert abs(float(mel.hz_to_mel(8000.0)) - 45.245640471924965) < 1e-9
    assert abs(float(mel.hz_to_mel(500.0)) - 7.5) < 1e-12                 # linear part: 200 / 3 Hz per mel
    f = np.array([0.0, 300.0, 999.0, 1000.0, 4321.0, 11025.0])
    assert np.allclose(mel.mel_to_hz(mel.hz_to_mel(f)), f, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('fmax', [8000.0, None])
def test_filter_bank_triangles_peaks_and_area(fmax):
    sr, n_fft, n_mels = 22050, 1024, 80
    fb = mel.mel_filter_bank(sr, n_fft, n_mels, 0.0, fmax)
    assert fb.shape == (80, 513) and fb.dtype == np.float32
    top = sr / 2 if fmax is None else fmax
    mel_f = mel.mel_to_hz(np.linspace(0.0, mel.hz_to_mel(top), n_mels + 2))
    freqs = np.fft.rfftfreq(n_fft, 1.0 / sr)
    df = freqs[1]
    for i in range(n_mels):
        lo, c, hi = mel_f[i], mel_f[i + 1], mel_f[i + 2]
        enorm = 2.0 / (hi - lo)
        nz = np.flatnonzero(fb[i])
        assert nz.size > 0, i
        assert freqs[nz[0]] > lo and freqs[nz[-1]] < hi                # support strictly inside (lo, hi)
        k = int(np.argmax(fb[i]))
        assert abs(freqs[k] - c) <= df, (i, freqs[k], c)                 # peak at the bin nearest the mel-spaced centre
        tri = np.maximum(0, np.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c)))
        assert np.allclose(fb[i], (tri.astype(np.float32).astype(np.float64) * enorm).astype(np.float32), rtol=1e-6, atol=0)
        assert fb[i].max() <= enorm * (1 + 1e-6)                          # Slaney height 2 / (f[i+2] - f[i])
        if hi - lo > 20 * df:                                             # unit area once the triangle spans many bins
            assert abs(fb[i].sum() * df - 1.0) < 0.02, (i, fb[i].sum() * df)


def test_filter_bank_zero_columns_above_kmax():
    fb = mel.mel_filter_bank(22050, 1024, 80, 0.0, 8000.0)
    assert not fb[:, 372:].any() and fb[:, 371].any()
    full = mel.mel_filter_bank(22050, 1024, 80, 0.0, None)
    assert not full[:, 512].any() and full[:, 1:512].any(axis=0).all()
    assert mel.MelSpectrogram().kmax == 372 and mel.MelSpectrogram(fmax=None).kmax == 512


def test_filter_bank_is_cached_and_returned_as_a_copy():
    a = mel.mel_filter_bank(22050, 1024, 80, 0, 8000)
    a[:] = 0
    assert mel.mel_filter_bank(22050, 1024, 80, 0, 8000).any()


@pytest.mark.parametrize('n', [385, 512, 1000, 22050, 44101])
def test_frame_count_matches_torch_stft(n):
    x = torch.randn(n)
    xp = torch.nn.functional.pad(x[None, None], (384, 384), mode='reflect')[0, 0]
    spec = torch.stft(xp, 1024, hop_length=256, win_length=1024, window=torch.hann_window(1024), center=False, return_complex=True)
    assert spec.shape[-1] == mel.n_frames(n) == n // 256


def test_arguments_are_checked_before_any_launch():
    with pytest.raises(ValueError):
        mel.check_lengths([1000, 384], 1000)
    with pytest.raises(ValueError):
        mel.check_lengths([1001], 1000)
    mel.check_lengths([385, 1000], 1000)
    with pytest.raises(ValueError):
        mel.mel_spectrogram_HiFi(np.zeros(384, dtype=np.float32), None)
    with pytest.raises(ValueError):
        mel.mel_spectrogram(torch.zeros(2, 300), 1024, 80, 22050, 256, 1024, 0, 8000)
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(torch.zeros(1, 4096), 1024, 80, 22050, 256, 1024, 0, None, center=True)
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(torch.zeros(1, 4096), 2048, 80, 22050, 256, 2048, 0, None)
    with pytest.raises(NotImplementedError):
        mel.mel_spectrogram(torch.zeros(1, 4096), 1024, 80, 22050, 128, 1024, 0, None)
    with pytest.raises(NotImplementedError):
        mel.MelSpectrogram(type('H', (), {'filter_length': 512})())
    with pytest.raises(ValueError):
        mel.MelSpectrogram(device='cpu')(torch.zeros(1, 4096), [4096])  # no CPU path


def test_mel_launch_is_priced_on_valid_frames_only():
    frames = [129, 40, 3]
    geom = profiling.Geometry([frames])
    a = dict(B=3, T_max=129, n_mels=80, kmax=372, S=33054, sxb=33054, smb=80 * 129)
    label, bound, flops, byt = profiling.price('dx_mel', a, geom)
    assert label == 'mel<f32>' and bound == 'mfma'
    assert flops == 2.0 * sum(frames) * (1024 * 2 * 372 + 372 * 80)
    assert byt > 0


def test_fixture_is_self_consistent():
    g = mh.golden()
    assert {'speech', 'sine440', 'chirp_noise', 'noise_floor', 'edge385', 'edge511', 'edge512', 'edge513'} <= set(g)
    assert len(g['speech']['wav']) == 33054
    for name, d in g.items():
        n = len(d['wav'])
        for v, fmax in mh.FMAX.items():
            e = d[v]
            assert e['ref'].shape == e['f64'].shape == (80, n // 256), (name, v)
            assert e['energy_ref'].shape == e['energy_f64'].shape == (n // 256,)
            m64, e64 = mh.mel_fp64(d['wav'], mel.mel_filter_bank(22050, 1024, 80, 0.0, fmax))
            assert np.allclose(m64, e['f64'], rtol=0, atol=1e-12) and np.allclose(e64, e['energy_f64'], rtol=1e-12, atol=0)
            dm, de = np.abs(e['ref'] - e['f64']), np.abs(e['energy_ref'] - e['energy_f64'])
            assert np.allclose(e['spread'], [dm.max(), dm.mean(), de.max(), de.mean()], rtol=1e-12, atol=0)
            assert np.allclose(e['energy_ref'], np.linalg.norm(np.exp(e['ref'].astype(np.float64)), axis=0), rtol=1e-5)
            assert e['spread'][0] < 5e-3 and e['ref'].min() >= np.log(1e-5) - 1e-6
