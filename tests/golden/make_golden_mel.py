"""Writes tests/golden/mel_frontend.npz from the REFERENCE mel extraction (extract_features.mel_spectrogram_HiFi, fmax 8000, and
vocoder/dataset.mel_spectrogram, fmax None, both center=False) on CPU.

Runs only where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.  The reference modules are
loaded from their files under an empty parent package (so daft_exprt/__init__.py never runs) with a stub ``librosa`` whose
``filters.mel`` is this package's ``mel_filter_bank`` (librosa is not installed).  Per signal the fixture holds the input (int16 for
the recording, float32 otherwise), the reference's fp32 log-mel and energy (``extract_energy(np.exp(mel))``), the fp64 restatement
(tests/mel_helpers.mel_fp64) and the spread of the reference against it: [mel max, mel mean, energy max, energy mean] of |fp32 - fp64|.

    python tests/golden/make_golden_mel.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from scipy.io import wavfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
SRC = '/root/reference/src/daft_exprt'
WAV = '/root/reference/scripts/style_bank/english/0_audio_ref.wav'

from tests.mel_helpers import FMAX, mel_fp64  # noqa: E402
from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank  # noqa: E402

torch.set_num_threads(8)


def _load_reference():
    pkg = types.ModuleType('daft_exprt')
    pkg.__path__ = [SRC]
    sys.modules['daft_exprt'] = pkg
    librosa = types.ModuleType('librosa')
    filters = types.ModuleType('librosa.filters')
    filters.mel = lambda sr, n_fft, n_mels=128, fmin=0.0, fmax=None, **kw: mel_filter_bank(sr, n_fft, n_mels, fmin, fmax)
    librosa.filters = filters
    sys.modules['librosa'], sys.modules['librosa.filters'] = librosa, filters
    mods = []
    for name, path in (('daft_exprt.extract_features', os.path.join(SRC, 'extract_features.py')),
                       ('ref_vocoder_dataset', os.path.join(SRC, 'vocoder', 'dataset.py'))):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def signals():
    _, speech = wavfile.read(WAV)
    assert speech.dtype == np.int16 and len(speech) == 33054
    g = np.random.default_rng(1234)
    n = np.arange(8192)
    sr = 22050.0
    f0, f1 = 100.0, 8000.0
    chirp = 0.5 * np.sin(2 * np.pi * (f0 * n / sr + (f1 - f0) * (n / sr) ** 2 / (2 * 8192 / sr))) + 1e-3 * g.standard_normal(8192)
    out = {'speech': speech,
           'sine440': (0.5 * np.sin(2 * np.pi * 440.0 * n / sr)).astype(np.float32),
           'chirp_noise': chirp.astype(np.float32),
           'noise_floor': (1e-4 * g.standard_normal(8192)).astype(np.float32)}
    for L in (385, 511, 512, 513):
        out[f'edge{L}'] = speech[12000:12000 + L]
    return out


def main():
    ef, ds = _load_reference()
    hp = types.SimpleNamespace(mel_fmin=0.0, mel_fmax=8000.0, hop_length=256, filter_length=1024, n_mel_channels=80,
                               sampling_rate=22050, min_clipping=1e-5)
    rec = {}
    names = []
    for name, x in signals().items():
        names.append(name)
        rec[f'{name}/wav'] = x
        wav = x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x
        for v, fmax in FMAX.items():
            with torch.no_grad():
                if v == 'hifi':
                    ref = ef.mel_spectrogram_HiFi(wav, hp)
                else:
                    ref = ds.mel_spectrogram(torch.from_numpy(wav)[None], 1024, 80, 22050, 256, 1024, 0.0, None, center=False)[0].numpy()
            ref = ref.reshape(80, -1).astype(np.float32)
            e_ref = ef.extract_energy(np.exp(ref)).astype(np.float32)
            m64, e64 = mel_fp64(wav, mel_filter_bank(22050, 1024, 80, 0.0, fmax))
            assert ref.shape == m64.shape == (80, len(wav) // 256), (name, ref.shape, m64.shape)
            dm, de = np.abs(ref - m64), np.abs(e_ref - e64)
            spread = np.array([dm.max(), dm.mean(), de.max(), de.mean()])
            rec.update({f'{name}/{v}/ref': ref, f'{name}/{v}/f64': m64, f'{name}/{v}/energy_ref': e_ref, f'{name}/{v}/energy_f64': e64,
                        f'{name}/{v}/spread': spread})
            print(f'{name:12s} {v}: T {ref.shape[1]:4d}  |ref32 - f64| mel max {dm.max():.2e} mean {dm.mean():.2e}  '
                  f'energy max {de.max():.2e} mean {de.mean():.2e}')
    rec['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'mel_frontend.npz'), **rec)


if __name__ == '__main__':
    main()
