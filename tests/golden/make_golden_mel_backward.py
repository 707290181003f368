"""Writes the backward fixture of the mel front end from the REFERENCE's own mel_spectrogram (vocoder/dataset.py, center=False, fmax 8000
and None) on CPU: tests/golden/mel_backward.npz and the per-sample arrays in mel_backward_{grad,loss}_{hifi,full}.npz (one file would
pass the 1 MiB limit on committed files).

Runs only where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.  The reference module is loaded
as in make_golden_mel.py: from its file, under an empty parent package, with a stub ``librosa`` whose ``filters.mel`` is this package's
``mel_filter_bank``.  Inputs are the signals of mel_frontend.npz.  Per signal and variant:

  g            seeded N(0, 1) upstream gradient (80, T), zeroed where the fp64 linear mel lies within a relative 1e-2 of the clip
               (an fp32 and an fp64 clamp may disagree there); ``share`` is the fraction zeroed
  d64          d(sum g . mel) / d(wav) by autograd through the fp64 restatement (tests/mel_grad_helpers.py)
  d32_ref      the same through the reference's mel_spectrogram in fp32;  spread = [max, mean] |d32_ref - d64|
  target       the fp64 log-mel of 0.9 wav + 0.01 noise, stored in float32
  loss_ref     the reference's F.l1_loss(target, mel_spectrogram(wav)) * 45 in fp32; loss64 the same in fp64
  dloss32_ref, dloss64   their waveform gradients;  loss_spread = [max, mean] |dloss32_ref - dloss64|

    python tests/golden/make_golden_mel_backward.py
"""
import importlib.util
import os
import sys
import types
import zlib

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
SRC = '/root/reference/src/daft_exprt'

from tests import mel_grad_helpers as gh  # noqa: E402
from tests import mel_helpers as mh  # noqa: E402
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
    spec = importlib.util.spec_from_file_location('ref_vocoder_dataset', os.path.join(SRC, 'vocoder', 'dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules['ref_vocoder_dataset'] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ds = _load_reference()
    ref_mel = lambda y, fmax: ds.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0.0, fmax, center=False)
    small, big = {}, {(k, v): {} for k in gh.BIG for v in mh.FMAX}
    names = []
    for name, d in mh.golden().items():
        names.append(name)
        wav = d['wav']
        for v, fmax in mh.FMAX.items():
            fb = mel_filter_bank(22050, 1024, 80, 0.0, fmax)
            rng = np.random.default_rng(zlib.crc32(f'{name}/{v}'.encode()))
            lin = gh.lin_fp64(wav, fb)
            near = gh.near_clip(lin)
            g = rng.standard_normal(lin.shape).astype(np.float32)
            g[near] = 0.0
            d64 = gh.grad_fp64(wav, fb, g)
            y = torch.from_numpy(wav)[None].requires_grad_(True)
            (ref_mel(y, fmax)[0] * torch.from_numpy(g)).sum().backward()
            d32 = y.grad[0].numpy().copy()
            dd = np.abs(d32 - d64)
            noise = rng.standard_normal(len(wav))
            target = gh.mel_fp64(0.9 * wav.astype(np.float64) + 0.01 * noise, fb).astype(np.float32)
            loss64, dl64 = gh.loss_fp64(wav, fb, target)
            y = torch.from_numpy(wav)[None].requires_grad_(True)
            loss = torch.nn.functional.l1_loss(torch.from_numpy(target)[None], ref_mel(y, fmax)) * 45
            loss.backward()
            dl32 = y.grad[0].numpy().copy()
            dl = np.abs(dl32 - dl64)
            small.update({f'{name}/{v}/g': g, f'{name}/{v}/share': np.float64(near.mean()), f'{name}/{v}/spread': np.array([dd.max(), dd.mean()]),
                          f'{name}/{v}/target': target, f'{name}/{v}/loss_ref': np.float32(loss.item()), f'{name}/{v}/loss64': np.float64(loss64),
                          f'{name}/{v}/loss_spread': np.array([dl.max(), dl.mean()])})
            big['grad', v].update({f'{name}/d64': d64, f'{name}/d32_ref': d32})
            big['loss', v].update({f'{name}/dloss64': dl64, f'{name}/dloss32_ref': dl32})
            clamped = (lin < gh.CLIP).mean()
            print(f'{name:12s} {v}: T {lin.shape[1]:4d} clamped {clamped:.3f} zeroed {near.mean():.4f}  grad rel max {dd.max() / np.abs(d64).max():.2e} '
                  f'mean {dd.mean() / np.abs(d64).max():.2e}  loss {loss64:.6f} (ref32 {loss.item():.6f})  loss grad rel max '
                  f'{dl.max() / np.abs(dl64).max():.2e}')
    small['names'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'mel_backward.npz'), **small)
    for (k, v), rec in big.items():
        np.savez_compressed(os.path.join(HERE, f'mel_backward_{k}_{v}.npz'), **rec)


if __name__ == '__main__':
    main()
