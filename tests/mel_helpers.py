"""Fixture loading and the fp64 restatement of the mel front end for the mel tests (numpy only; nothing here reads the reference tree)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FMAX = {'hifi': 8000.0, 'full': None}        # mel_spectrogram_HiFi (fmax 8000) and the vocoder's loss mel (full band)


def mel_fp64(wav, fb, clip=1e-5):
    """One utterance in float64: reflect pad 384, frames of 1024 / hop 256 under the periodic Hann window, sqrt(|X|^2 + 1e-9),
    fb (float32 values) @ mag, log(max(., clip)); energy = L2 norm of the clamped mel over channels.  -> (log-mel (n_mels, T), energy (T,))."""
    x = np.asarray(wav, dtype=np.float64)
    x = np.pad(x, (384, 384), mode='reflect')
    T = (len(x) - 1024) // 256 + 1
    idx = np.arange(1024)[None, :] + 256 * np.arange(T)[:, None]
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    spec = np.fft.rfft(x[idx] * win, axis=1)
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    mel = np.maximum(fb.astype(np.float64) @ mag.T, clip)
    return np.log(mel), np.sqrt((mel ** 2).sum(axis=0))


def golden():
    """-> {name: {'wav': float32 (S,), 'hifi'/'full': {'ref', 'f64', 'energy_ref', 'energy_f64', 'spread'}}} from mel_frontend.npz."""
    z = np.load(os.path.join(GOLDEN, 'mel_frontend.npz'))
    out = {}
    for name in [str(n) for n in z['names']]:
        wav = z[f'{name}/wav']
        wav = wav.astype(np.float32) / 32768.0 if wav.dtype == np.int16 else wav.astype(np.float32)
        d = {'wav': wav}
        for v in FMAX:
            d[v] = {k: z[f'{name}/{v}/{k}'] for k in ('ref', 'f64', 'energy_ref', 'energy_f64', 'spread')}
        out[name] = d
    return out
