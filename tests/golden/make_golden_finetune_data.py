"""Writes tests/golden/finetune_data.npz and finetune_data_manifest.json from the REFERENCE's vocoder/dataset.py
``HiFiGANFinetuneDataset`` and ``torch.utils.data.random_split`` as vocoder/finetune_hifigan.py:155-165 calls them, on the synthetic
tree of tests/finetune_data_helpers.py (segment_size 2048: 8 frames per segment).

Runs only where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.  The reference module is loaded
from its file as make_golden_mel.py loads it: with a stub ``librosa`` whose ``filters.mel`` is this package's ``mel_filter_bank``, and
with scipy's wav reader.  The manifest records the shuffled pair order and the members of the train and validation subsets (wav paths
relative to the tree); the npz the reference's ``(mel, audio, mel_loss)`` of the helper's ITEMS with ``random.randint`` patched to
return the recorded start (and to check the range it was asked for).

    python tests/golden/make_golden_finetune_data.py
"""
import importlib.util
import json
import os
import random
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
SRC = '/root/reference/src/daft_exprt'

from tests import finetune_data_helpers as fh  # noqa: E402
from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank  # noqa: E402

torch.set_num_threads(8)
VAL_SPLIT = 0.1


def _load_reference():
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
    with tempfile.TemporaryDirectory() as root:
        fh.write_tree(root)
        rel = lambda p: os.path.relpath(p, root).replace(os.sep, '/')
        data = ds.HiFiGANFinetuneDataset(root, fh.SEGMENT, 1024, 80, fh.HOP, 1024, fh.SR, 0, 8000, split=True, shuffle=True,
                                         fmax_loss=None, device=None)
        n_total = len(data)
        n_val = max(1, int(n_total * VAL_SPLIT))
        n_train = n_total - n_val
        train_set, val_set = torch.utils.data.random_split(data, [n_train, n_val], generator=torch.Generator().manual_seed(1234))
        pairs = [rel(w) for _, w in data.pairs]
        man = {'segment_size': fh.SEGMENT, 'hop_size': fh.HOP, 'sampling_rate': fh.SR, 'val_split': VAL_SPLIT, 'pairs': pairs,
               'train': [pairs[i] for i in train_set.indices], 'val': [pairs[i] for i in val_set.indices],
               'items': [[stem + '.wav', start] for stem, start in fh.ITEMS]}
        rec = {}
        real_randint = random.randint
        try:
            for k, (stem, start) in enumerate(fh.ITEMS):
                index = pairs.index(stem + '.wav')
                asked = []
                random.randint = lambda a, b, start=start, asked=asked: (asked.append((a, b)), start)[1]
                with torch.no_grad():
                    mel, audio, wav_path, mel_loss = data[index]
                assert rel(wav_path) == stem + '.wav'
                assert all(a <= start <= b for a, b in asked), (stem, start, asked)
                assert mel.shape == (80, fh.FPS) and audio.shape == (fh.SEGMENT,) and mel_loss.shape == (80, fh.FPS), (stem, mel.shape)
                rec[f'{k}/mel'], rec[f'{k}/audio'], rec[f'{k}/mel_loss'] = mel.numpy(), audio.numpy(), mel_loss.numpy()
                print(f'{stem:14s} start {start:3d}  randint asked {asked}')
        finally:
            random.randint = real_randint
    np.savez_compressed(os.path.join(HERE, 'finetune_data.npz'), **rec)
    with open(os.path.join(HERE, 'finetune_data_manifest.json'), 'w') as f:
        json.dump(man, f, indent=1)
        f.write('\n')
    print(f'{n_total} pairs: {n_train} train, {n_val} val')


if __name__ == '__main__':
    main()
