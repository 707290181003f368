"""The HiFi-GAN fine-tuning data on the device (reference vocoder/dataset.py:67-156 ``HiFiGANFinetuneDataset`` and
vocoder/finetune_hifigan.py:154-175, the split and the two loaders): the whole corpus is uploaded once, ``dx_ft_batch`` crops a batch in
one launch and the existing mel front end makes the loss mel in a second one.  No host work, no host-to-device copy and no
synchronisation per step.

Pair discovery, the shuffle and the train / validation split are the reference's, bit for bit (``train_names`` / ``val_names`` are its
``train_set`` / ``val_set`` members in order).  What a step sees is a function of ``(seed, step)`` alone: the pass of step ``s`` is
``s // steps_per_epoch``, the order of pass ``e`` is ``torch.randperm`` seeded from ``(seed, e)``, and the crop start of row ``b`` is drawn
in the kernel from ``dx_rand64(seed, (s << 20) | b)``.

Stated deviations from the reference: a pair the reference would fail on later, inside a worker (``T_mel - fps - 1 < 0``: its ``randint``
raises), or would turn into a ragged item (audio shorter than ``(T_mel - 1) * hop``: its slice comes out short) is a ``ValueError`` at
construction that names the file, and so are a wav that is not 16-bit mono PCM at ``sampling_rate``, fewer training pairs than
``batch_size`` (the reference spins forever on an empty loader) and a corpus larger than ``max_bytes``; the start is
``(uint32 draw * n) >> 32``, biased by at most ``2^-32 n``; validation crops come from a separate counter stream keyed by the utterance
alone, so every validation sees the same crops (the reference redraws them).
"""
from __future__ import annotations

import math
import os
import random
import wave

import numpy as np
import torch

from ._lib import lib
from .mel import HOP, MelSpectrogram

N_MELS = 80
SPLIT_SEED = 1234                      # the reference's random.seed(1234) and random_split(generator=manual_seed(1234))
VAL_TAG = 1 << 63                      # the counter bit of the validation stream
_MASK64 = (1 << 64) - 1


def find_pairs(root_dir):
    """vocoder/dataset.py:67-78: every ``.wav`` with a ``.npy`` of the same stem -> [(mel_path, wav_path)] sorted by wav path."""
    pairs = []
    for dirpath, _dirs, files in os.walk(root_dir):
        for wf in sorted(f for f in files if f.endswith('.wav')):
            mel_path = os.path.join(dirpath, os.path.splitext(wf)[0] + '.npy')
            if os.path.isfile(mel_path):
                pairs.append((mel_path, os.path.join(dirpath, wf)))
    pairs.sort(key=lambda p: p[1])
    return pairs


def read_wav_int16(path, sampling_rate):
    """16-bit mono PCM at ``sampling_rate`` -> int16 (n,); anything else is a ValueError that names the file."""
    try:
        with wave.open(path, 'rb') as w:
            fmt = (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getcomptype())
            raw = w.readframes(w.getnframes())
    except (wave.Error, EOFError) as exc:
        raise ValueError(f'{path}: not a PCM wav file ({exc})') from None
    if fmt[:2] != (1, 2) or fmt[3] != 'NONE':
        raise ValueError(f'{path}: expected 16-bit mono PCM, got {fmt[0]} channel(s) of {8 * fmt[1]} bits')
    if fmt[2] != sampling_rate:
        raise ValueError(f'{path}: sample rate {fmt[2]} != expected {sampling_rate}')
    return np.frombuffer(raw, dtype='<i2').astype(np.int16)


def read_mel(path):
    """``(80, T)`` or ``(1, 80, T)`` -> float32 (80, T)."""
    mel = np.load(path)
    shape = tuple(mel.shape)
    if mel.ndim == 3 and mel.shape[0] == 1:
        mel = mel[0]
    if mel.ndim != 2 or mel.shape[0] != N_MELS:
        raise ValueError(f'{path}: expected a ({N_MELS}, T) or (1, {N_MELS}, T) mel, got shape {shape}')
    return np.ascontiguousarray(mel, dtype=np.float32)


def pass_seed(seed, epoch):
    """The 63-bit seed of pass ``epoch``'s order: a splitmix64 finaliser over ``(seed, epoch)``."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + (int(epoch) + 1) * 0xD1B54A32D192ED03) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return (z ^ (z >> 31)) >> 1


class HiFiGanFineTuneData:
    """``root_dir``: a tree of ``.npy`` (predicted mel) / ``.wav`` pairs as the reference's ``fine_tune.py`` writes it.  ``max_bytes``:
    the largest resident corpus accepted (None: no limit).  With ``device`` on the GPU the corpus is uploaded at construction; on the
    CPU the object answers only the host questions (names, splits, orders) and ``batch`` raises.

    Public: ``names`` (wav paths in the reference's shuffled order: utterance ``u`` of every index below), ``train_indices``,
    ``val_indices``, ``train_names``, ``val_names``, ``steps_per_epoch``, ``nbytes``, ``wav_lengths``, ``mel_lengths``."""

    def __init__(self, root_dir, segment_size=8192, hop_size=HOP, sampling_rate=22050, val_split=0.1, batch_size=16, seed=0,
                 device='cuda', max_bytes=None):
        pairs = find_pairs(root_dir)
        if not pairs:
            raise RuntimeError(f'No mel/wav pairs found in {root_dir}. Expected .npy and .wav files with matching stems.')
        random.Random(SPLIT_SEED).shuffle(pairs)                       # = random.seed(1234); random.shuffle(pairs)
        mels = [read_mel(m) for m, _ in pairs]
        wavs = [read_wav_int16(w, int(sampling_rate)) for _, w in pairs]
        self._init([w for _, w in pairs], mels, wavs, segment_size, hop_size, sampling_rate, val_split, batch_size, seed, device, max_bytes)

    @classmethod
    def from_arrays(cls, names, mels, wavs_int16, segment_size=8192, hop_size=HOP, sampling_rate=22050, val_split=0.1, batch_size=16,
                    seed=0, device='cuda', max_bytes=None):
        """The corpus from memory: ``names[u]``, ``mels[u]`` ((80, T) or (1, 80, T)) and ``wavs_int16[u]`` (int16 (n,)) are utterance
        ``u`` of the data set as it is indexed (the directory constructor's order after its shuffle; nothing is shuffled here)."""
        self = cls.__new__(cls)
        if not len(names):
            raise RuntimeError('No mel/wav pairs given.')
        if not len(names) == len(mels) == len(wavs_int16):
            raise ValueError(f'{len(names)} names, {len(mels)} mels and {len(wavs_int16)} wavs')
        host_mels, host_wavs = [], []
        for name, m, w in zip(names, mels, wavs_int16):
            m, w = np.asarray(m), np.asarray(w)
            if m.ndim == 3 and m.shape[0] == 1:
                m = m[0]
            if m.ndim != 2 or m.shape[0] != N_MELS:
                raise ValueError(f'{name}: expected a ({N_MELS}, T) or (1, {N_MELS}, T) mel, got shape {tuple(m.shape)}')
            if w.dtype != np.int16 or w.ndim != 1:
                raise ValueError(f'{name}: expected int16 samples (n,), got {w.dtype} {tuple(w.shape)}')
            host_mels.append(np.ascontiguousarray(m, dtype=np.float32))
            host_wavs.append(w)
        self._init(list(names), host_mels, host_wavs, segment_size, hop_size, sampling_rate, val_split, batch_size, seed, device, max_bytes)
        return self

    def _init(self, names, mels, wavs, segment_size, hop_size, sampling_rate, val_split, batch_size, seed, device, max_bytes):
        self.segment_size, self.hop_size, self.sampling_rate = int(segment_size), int(hop_size), int(sampling_rate)
        self.batch_size, self.seed, self.device = int(batch_size), int(seed) & _MASK64, torch.device(device)
        if self.hop_size != HOP:
            raise NotImplementedError(f'the loss mel is the gfx950 front end: hop_size must be {HOP}, got {hop_size}')
        if self.segment_size < self.hop_size or self.segment_size % self.hop_size:
            raise ValueError(f'segment_size {segment_size} must be a whole number of hops of {hop_size} samples')
        if not 1 <= self.batch_size <= 1 << 20:
            raise ValueError(f'batch_size {batch_size} must be in [1, 2^20] (the row is the low 20 bits of the draw counter)')
        self.fps = math.ceil(self.segment_size / self.hop_size)
        self.names = list(names)
        n = len(self.names)
        for name, m, w in zip(self.names, mels, wavs):
            if len(w) < self.segment_size:
                continue                                              # padded with zeros, never cropped
            if m.shape[1] - self.fps - 1 < 0:
                raise ValueError(f'{name}: {len(w)} samples reach segment_size but the mel has {m.shape[1]} frames; a crop needs at least '
                                 f'{self.fps + 1} (the reference\'s randint(0, T_mel - {self.fps} - 1) raises)')
            if len(w) < (m.shape[1] - 1) * self.hop_size:
                raise ValueError(f'{name}: {len(w)} samples for a mel of {m.shape[1]} frames; the last crop needs '
                                 f'{(m.shape[1] - 1) * self.hop_size} (the reference\'s audio slice would come out short)')
        # finetune_hifigan.py:160-165: random_split of [n_train, n_val] under manual_seed(1234)
        n_val = max(1, int(n * val_split))
        n_train = n - n_val
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(SPLIT_SEED)).tolist()
        self.train_indices, self.val_indices = perm[:n_train], perm[n_train:]
        if n_train < self.batch_size:
            raise ValueError(f'{n_train} training pairs ({n} found, {n_val} held out for validation) do not fill one batch of {batch_size}: '
                             'with drop_last the loader would be empty')
        self.train_names = [self.names[i] for i in self.train_indices]
        self.val_names = [self.names[i] for i in self.val_indices]
        self.steps_per_epoch = n_train // self.batch_size              # drop_last=True
        self.wav_lengths = [len(w) for w in wavs]
        self.mel_lengths = [m.shape[1] for m in mels]
        # resident layout: utterance u's samples at wav_off[u] (a multiple of 8 samples = 16 bytes; the padding after it is zeros),
        # its mel as (80, T_u) at mel_off[u]
        wav_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([(len(w) + 7) // 8 * 8 for w in wavs], out=wav_off[1:])
        mel_off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([m.size for m in mels], out=mel_off[1:])
        self.nbytes = int(wav_off[-1]) * 2 + int(mel_off[-1]) * 4 + n * (8 + 8 + 4 + 4)
        if max_bytes is not None and self.nbytes > max_bytes:
            raise ValueError(f'the corpus needs {self.nbytes} bytes on the device, more than max_bytes = {max_bytes}')
        self._orders = {}
        self._val = None
        self._mel = None
        self._tables = None
        if self.device.type == 'cuda':
            wav_buf = np.zeros(int(wav_off[-1]), dtype=np.int16)
            mel_buf = np.empty(int(mel_off[-1]), dtype=np.float32)
            for u, (m, w) in enumerate(zip(mels, wavs)):
                wav_buf[wav_off[u]:wav_off[u] + len(w)] = w
                mel_buf[mel_off[u]:mel_off[u + 1]] = m.reshape(-1)
            up = lambda a: torch.from_numpy(a).to(self.device)
            self._tables = (up(wav_buf), up(wav_off[:-1].copy()), up(np.asarray(self.wav_lengths, dtype=np.int32)),
                            up(mel_buf), up(mel_off[:-1].copy()), up(np.asarray(self.mel_lengths, dtype=np.int32)))
            self._mel = MelSpectrogram(fmax=None, device=self.device)  # the reference's FMAX_FOR_LOSS = None

    # ---- order: host, a function of (seed, step) ----------------------------------------------------------------------------------
    def epoch_of(self, step):
        """-> (pass, position inside the pass) of step ``step`` (0-based: the step that takes the tuner from ``step`` to ``step + 1``)."""
        return int(step) // self.steps_per_epoch, int(step) % self.steps_per_epoch

    def epoch_order(self, epoch):
        """The utterances of pass ``epoch`` in the order they are used, int32 (n_train,); its first ``steps_per_epoch * batch_size``
        entries are the pass's batches (the rest is what ``drop_last`` drops)."""
        perm = torch.randperm(len(self.train_indices), generator=torch.Generator().manual_seed(pass_seed(self.seed, epoch)))
        return torch.tensor(self.train_indices, dtype=torch.int32)[perm]

    def _order(self, epoch):
        if epoch not in self._orders:
            if len(self._orders) >= 2:                                 # kept: the pass in progress and, across a boundary, its neighbour
                self._orders.pop(max(self._orders, key=lambda e: abs(e - epoch)))
            pinned = self.epoch_order(epoch).pin_memory()
            self._orders[epoch] = (pinned.to(self.device, non_blocking=True), pinned)   # the host copy lives as long as the device one
        return self._orders[epoch][0]

    # ---- batches: device -----------------------------------------------------------------------------------------------------------
    def _launch(self, B, utts, order, order_pos, starts, counter, by_utt):
        if self._tables is None:
            raise RuntimeError('HiFiGanFineTuneData assembles batches on the GPU (gfx950 HIP kernel); there is no CPU path')
        wav, wav_off, wav_len, mel, mel_off, mel_len = self._tables
        dev = self.device
        x = torch.empty(B, N_MELS, self.fps, dtype=torch.float32, device=dev)
        y = torch.empty(B, self.segment_size, dtype=torch.float32, device=dev)
        starts_out = torch.empty(B, dtype=torch.int32, device=dev)
        utts_out = torch.empty(B, dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()
        lib().dx_ft_batch(wav.data_ptr(), wav_off.data_ptr(), wav_len.data_ptr(), mel.data_ptr(), mel_off.data_ptr(), mel_len.data_ptr(),
                          len(self.names), ptr(utts), ptr(order), order_pos, 0 if order is None else order.numel(), ptr(starts), self.seed,
                          counter, by_utt, x.data_ptr(), y.data_ptr(), starts_out.data_ptr(), utts_out.data_ptr(), B, self.segment_size,
                          self.hop_size, self.fps, N_MELS, torch.cuda.current_stream(dev).cuda_stream)
        y_mel, _, _ = self._mel(y, [self.segment_size] * B)
        return x, y, y_mel, starts_out, utts_out

    def batch(self, step):
        """The training batch of step ``step`` -> (x (B, 80, fps), y (B, segment_size), y_mel (B, 80, fps), starts (B,) int32, utts (B,)
        int32), all on the device: two launches, nothing read back."""
        step = int(step)
        if not 0 <= step < 1 << 43:
            raise ValueError(f'step {step} must be in [0, 2^43)')
        epoch, pos = self.epoch_of(step)
        return self._launch(self.batch_size, None, self._order(epoch), pos * self.batch_size, None, step << 20, 0)

    def val_batches(self):
        """Yields (x, y_mel) over the validation utterances in ``val_indices`` order, at most ``batch_size`` per batch; the crops are
        the same at every call."""
        if self._val is None:
            self._val = torch.tensor(self.val_indices, dtype=torch.int32).to(self.device)
        for i in range(0, len(self.val_indices), self.batch_size):
            B = min(self.batch_size, len(self.val_indices) - i)
            x, _, y_mel, _, _ = self._launch(B, self._val[i:i + B], None, 0, None, VAL_TAG, 1)
            yield x, y_mel

    def max_start(self, utt):
        """The largest crop start of utterance ``utt``: ``T_mel - fps - 1``, or 0 for an utterance shorter than the segment."""
        return 0 if self.wav_lengths[utt] < self.segment_size else self.mel_lengths[utt] - self.fps - 1

    def assemble(self, utts, starts):
        """Rows given explicitly (host integers): utterance ``utts[b]`` cropped at frame ``starts[b]`` -> the tuple of ``batch``."""
        utts, starts = [int(u) for u in utts], [int(s) for s in starts]
        if not utts or len(utts) != len(starts):
            raise ValueError(f'{len(utts)} utterances and {len(starts)} starts')
        for u, s in zip(utts, starts):
            if not 0 <= u < len(self.names):
                raise ValueError(f'utterance {u} is outside [0, {len(self.names)})')
            if not 0 <= s <= self.max_start(u):
                raise ValueError(f'{self.names[u]}: start {s} is outside [0, {self.max_start(u)}]')
        to = lambda v: torch.tensor(v, dtype=torch.int32).to(self.device)
        return self._launch(len(utts), to(utts), None, 0, to(starts), 0, 0)


__all__ = ['HiFiGanFineTuneData', 'find_pairs', 'read_wav_int16', 'read_mel', 'pass_seed', 'N_MELS', 'VAL_TAG']
