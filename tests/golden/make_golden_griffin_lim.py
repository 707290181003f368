"""Writes tests/golden/griffin_lim.npz from the REFERENCE Griffin-Lim vocoding (griffin_lim.py: mel_to_linear and
reconstruct_signal_griffin_lim) on CPU, in float64 as the reference runs it.

Runs only where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.  The reference module is loaded
from its file under an empty parent package with a stub ``librosa`` whose ``filters.mel`` is this package's ``mel_filter_bank`` (librosa
is not installed).  The start noise is drawn once here, rounded to float32, stored, and handed to the reference by patching the
``np.random.randn`` call it makes.

Contents.  Two log-mels from mel_frontend.npz (a 40-frame crop of speech/hifi, the chirp_noise mel); for each the reference's NNLS
solution (rounded to float32) and its relative residual |A X - m| / |m| (of the float64 solution).  From the speech solution as float32
magnitudes, last two frames dropped (38 frames): the reference's signal after 1, 8 and 32 iterations from the stored noise and from an
all-zero start (which exercises angle(0) = 0), the spectral convergence | |STFT(x)| - M | / |M| after 128 iterations from the noise, and
the float32 spread at each of those points: the same steps in float32 (tests/griffin_lim_helpers, scipy.fft) against float64, as
[max |x32 - x64|, |x32 - x64|_2 / |x64|_2].  The archive is written with fixed timestamps, so it regenerates bit for bit.

    python tests/golden/make_golden_griffin_lim.py
"""
import importlib.util
import io
import os
import sys
import types
import zipfile

sys.dont_write_bytecode = True

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
SRC = '/root/reference/src/daft_exprt'

from tests import griffin_lim_helpers as gh  # noqa: E402
from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank  # noqa: E402

CROP = (30, 70)               # frames of speech/hifi
LONG = 128


def _load_reference():
    pkg = types.ModuleType('daft_exprt')
    pkg.__path__ = [SRC]
    sys.modules['daft_exprt'] = pkg
    librosa = types.ModuleType('librosa')
    filters = types.ModuleType('librosa.filters')
    filters.mel = lambda sr, n_fft, n_mels=128, fmin=0.0, fmax=None, **kw: mel_filter_bank(sr, n_fft, n_mels, fmin, fmax)
    librosa.filters = filters
    sys.modules['librosa'], sys.modules['librosa.filters'] = librosa, filters
    spec = importlib.util.spec_from_file_location('daft_exprt.griffin_lim', os.path.join(SRC, 'griffin_lim.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['daft_exprt.griffin_lim'] = mod
    spec.loader.exec_module(mod)
    return mod


class _Quiet:
    def debug(self, *a, **k):
        pass


def _reference_signal(ref, M, start, iterations):
    """reconstruct_signal_griffin_lim from ``start`` in place of its own randn draw."""
    real = np.random.randn
    np.random.randn = lambda n: np.asarray(start[:n], dtype=np.float64).copy()
    try:
        x, _ = ref.reconstruct_signal_griffin_lim(M, 256, iterations, _Quiet())
    finally:
        np.random.randn = real
    return x


def save_npz(path, rec):
    """np.savez_compressed with fixed entry order and timestamps."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(rec):
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[k]), allow_pickle=False)
            z.writestr(info, buf.getvalue())


def main():
    ref = _load_reference()
    hp = types.SimpleNamespace(mel_fmin=0.0, mel_fmax=8000.0, hop_length=256, filter_length=1024, n_mel_channels=80, sampling_rate=22050)
    A = mel_filter_bank(22050, 1024, 80, 0.0, 8000.0)
    with np.load(os.path.join(HERE, 'mel_frontend.npz')) as d:
        mels = {'speech': np.ascontiguousarray(d['speech/hifi/ref'][:, CROP[0]:CROP[1]]), 'chirp': d['chirp_noise/hifi/ref'].copy()}
    rec = {}
    for name, mel in mels.items():
        lin = np.exp(mel)                                     # float32, as the reference's np.exp of a float32 mel
        X = ref.mel_to_linear(lin, hp)
        assert X.shape == (513, mel.shape[1]) and (X >= 0).all()
        res = gh.relative_residual(A, X, lin)
        rec[f'{name}/mel'], rec[f'{name}/nnls'], rec[f'{name}/residual'] = mel, X.astype(np.float32), np.float64(res)
        print(f'{name}: T {mel.shape[1]}  reference NNLS residual {res:.3e}')
    M = rec['speech/nnls'][:, :-2].astype(np.float64)          # the float32 magnitudes the device is given
    T = M.shape[1]
    S = 256 * T + 1024
    noise = np.random.default_rng(20240607).standard_normal(S).astype(np.float32)
    rec['noise'] = noise
    for start_name, start in (('noise', noise), ('zeros', np.zeros(S, dtype=np.float32))):
        _, x32 = gh.gl_iterate(M.astype(np.float32), start, max(gh.ITERS), np.float32, keep=gh.ITERS)
        _, x64 = gh.gl_iterate(M, start, max(gh.ITERS), np.float64, keep=gh.ITERS)
        for k in gh.ITERS:
            x = _reference_signal(ref, M, start, k)
            assert x.shape == (S,) and x.dtype == np.float64
            dev = np.abs(x64[k] - x).max()
            d32 = x32[k].astype(np.float64) - x
            spread = np.array([np.abs(d32).max(), np.linalg.norm(d32) / np.linalg.norm(x)])
            rec[f'gl/{start_name}/{k}'], rec[f'gl/{start_name}/{k}/spread'] = x, spread
            print(f'{start_name:5s} {k:3d} iterations: |restatement64 - reference| max {dev:.1e}; float32 spread max {spread[0]:.2e} rel L2 {spread[1]:.2e}')
    x = _reference_signal(ref, M, noise, LONG)
    sc64 = gh.spectral_convergence(x, M)
    sc32 = gh.spectral_convergence(gh.gl_iterate(M.astype(np.float32), noise, LONG, np.float32), M)
    rel = abs(sc32 - sc64) / sc64
    print(f'spectral convergence after {LONG}: reference {sc64:.6e}, float32 {sc32:.6e} (relative deviation {rel:.2e})')
    assert rel <= 2.5e-4, rel
    rec['gl/convergence'], rec['gl/convergence_f32'] = np.float64(sc64), np.float64(sc32)
    save_npz(os.path.join(HERE, 'griffin_lim.npz'), rec)


if __name__ == '__main__':
    main()
