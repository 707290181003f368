"""What the fine-tuning data tests share (numpy, the standard library and torch's CPU side only; nothing here reads the reference tree):
the deterministic synthetic corpus, the fixture's loader, numpy restatements of the kernel's draw and of the reference's per-item path,
the mel bar of tests/test_mel_gpu.py on the fixture's reference mels, and the seeded checkpoints of the fine-tuner tests."""
import functools
import json
import math
import os
import wave

import numpy as np

from tests import mel_helpers as mh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEGMENT, HOP, SR = 2048, 256, 22050
FPS = SEGMENT // HOP                     # 8

# (relative stem, mel frames T, samples n, mel stored as (1, 80, T)); the reference needs n >= (T - 1) * 256 of an utterance it crops
CORPUS = [
    ('a/utt00', 12, 12 * 256 + 17, False),
    ('a/utt01', 13, 13 * 256, False),                    # odd T_mel
    ('a/utt02', 5, 5 * 256 + 100, False),                # shorter than the segment: zero-padded, T_mel < fps
    ('a/utt03', 10, 10 * 256, True),                     # (1, 80, T) mel
    ('a/deep/utt04', 9, 8 * 256 + 3, False),             # T_mel - fps - 1 == 0: the only legal start is 0
    ('a/deep/utt05', 60, 60 * 256 + 255, False),         # the long one
    ('a/deep/utt06', 11, 11 * 256 - 256, False),         # exactly (T - 1) * hop samples
    ('b/utt07', 10, 2037, False),                        # short with T_mel > fps (F.pad crops the mel); 2037 is no multiple of 8
] + [(f'b/utt{k:02d}', 10 + (k * 7) % 9, (10 + (k * 7) % 9) * 256 + (k * 37) % 256, k % 5 == 0) for k in range(8, 16)] \
  + [(f'c/x/y/utt{k:02d}', 14 + (k * 5) % 11, (14 + (k * 5) % 11) * 256 - (k * 13) % 200, False) for k in range(16, 23)]
assert len(CORPUS) == 23

# the recorded items: (stem, start); start 0, the maximum start, an odd start, the forced 0, the two short ones, the (1, 80, T) mel
ITEMS = [('a/deep/utt05', 0), ('a/deep/utt05', 60 - FPS - 1), ('a/utt01', 3), ('a/deep/utt04', 0), ('a/utt02', 0), ('b/utt07', 0),
         ('a/utt03', 1)]


def utterance(stem, T, n, _three=False):
    """-> (mel float32 (80, T), int16 samples (n,)) of one synthetic utterance, from a seed that is the stem's own."""
    g = np.random.default_rng(int.from_bytes(stem.encode(), 'little') % (1 << 32))
    mel = (-5.0 + 2.0 * g.standard_normal((80, T))).astype(np.float32)
    t = np.arange(n) / SR
    wav = 0.4 * np.sin(2 * np.pi * (110.0 + 40.0 * g.random()) * t * (1.0 + 0.3 * t)) + 0.05 * g.standard_normal(n)
    pcm = np.clip(np.round(wav * 32767.0), -32768, 32767).astype(np.int16)
    pcm[0], pcm[-1] = -32768, 32767                       # both ends of the int16 range are in every file
    return mel, pcm


def write_tree(root, corpus=CORPUS):
    """Writes the corpus under ``root`` (nested directories), plus files the walk must ignore.  -> root."""
    for stem, T, n, three in corpus:
        mel, pcm = utterance(stem, T, n)
        path = os.path.join(root, *stem.split('/'))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.save(path + '.npy', mel[None] if three else mel)
        write_wav(path + '.wav', pcm)
    os.makedirs(os.path.join(root, 'extra'), exist_ok=True)
    write_wav(os.path.join(root, 'extra', 'no_mel.wav'), np.zeros(300, dtype=np.int16))     # a wav without a mel
    np.save(os.path.join(root, 'extra', 'no_wav.npy'), np.zeros((80, 4), dtype=np.float32))  # a mel without a wav
    return root


def write_wav(path, pcm, sr=SR, channels=1, width=2):
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(np.asarray(pcm).tobytes())


def arrays(stems):
    """-> (names, mels, wavs) of the corpus rows named by ``stems``, for ``HiFiGanFineTuneData.from_arrays``."""
    rows = {r[0]: r for r in CORPUS}
    pairs = [utterance(*rows[s]) for s in stems]
    return list(stems), [m for m, _ in pairs], [w for _, w in pairs]


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, 'finetune_data_manifest.json')) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def fixture():
    """finetune_data.npz: per recorded item k the reference's ``k/mel`` (80, fps), ``k/audio`` (segment,), ``k/mel_loss`` (80, fps)."""
    z = np.load(os.path.join(GOLDEN, 'finetune_data.npz'))
    return {k: z[k] for k in z.files}


# ---- the kernel's draw, restated -------------------------------------------------------------------------------------------------------
def rand64(seed, idx):
    """csrc/dx_common.h dx_rand64 on numpy uint64 arrays -> (high word, low word) as uint32."""
    seed, idx = np.uint64(seed), np.asarray(idx, dtype=np.uint64)
    u32 = lambda v: (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    with np.errstate(over='ignore'):
        x = u32(idx) ^ u32(seed)
        hi = u32(idx >> np.uint64(32)) ^ u32(seed >> np.uint64(32))
        x = x ^ (hi * np.uint32(0x9E3779B1))
        x ^= x >> np.uint32(16); x = x * np.uint32(0x7FEB352D); x ^= x >> np.uint32(15); x = x * np.uint32(0x846CA68B); x ^= x >> np.uint32(16)
        y = (x ^ np.uint32(0x85EBCA6B)) * np.uint32(0xC2B2AE35)
        y ^= y >> np.uint32(15)
    return y, x


def draw_start(seed, counter, n):
    """The start the kernel draws for a croppable utterance with ``n = T_mel - fps``: (high word * n) >> 32, in [0, n - 1]."""
    hi, _ = rand64(seed, counter)
    return ((hi.astype(np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def expected_starts(data, step, utts):
    """The starts of ``data.batch(step)`` for its rows' utterances, from the restated draw."""
    out = []
    for b, u in enumerate(utts):
        if data.wav_lengths[u] < data.segment_size:
            out.append(0)
        else:
            out.append(int(draw_start(data.seed, np.uint64((step << 20) | b), data.mel_lengths[u] - data.fps)))
    return out


# ---- the reference's per-item path, restated on the host (vocoder/dataset.py:118-148, without the loss mel) ---------------------------
def host_item(mel, pcm, start, segment=SEGMENT, hop=HOP):
    """-> (mel (80, fps), audio (segment,)) float32 as ``HiFiGANFinetuneDataset.__getitem__`` crops or pads them."""
    fps = math.ceil(segment / hop)
    audio = pcm.astype(np.float32) / 32768.0
    mel = np.asarray(mel, dtype=np.float32).reshape(80, -1)
    if len(audio) >= segment:
        return mel[:, start:start + fps].copy(), audio[start * hop:(start + fps) * hop].copy()
    T = mel.shape[1]
    x = np.zeros((80, fps), dtype=np.float32)
    x[:, :min(T, fps)] = mel[:, :fps]
    y = np.zeros(segment, dtype=np.float32)
    y[:len(audio)] = audio
    return x, y


def host_loss_mel(audio):
    """The reference's loss mel of one item on the host in fp32 (vocoder/dataset.py:26-64, fmax None): reflect pad 384, torch.stft
    1024 / 256 under the periodic Hann window, sqrt(|X|^2 + 1e-9), filter bank, log(clamp(1e-5)).  audio (segment,) -> (80, fps)."""
    import torch
    from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank
    y = torch.nn.functional.pad(torch.as_tensor(audio)[None, None], (384, 384), mode='reflect')[0]
    spec = torch.stft(y, 1024, hop_length=256, win_length=1024, window=torch.hann_window(1024), center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    return torch.log(torch.clamp(torch.from_numpy(mel_filter_bank(SR, 1024, 80, 0.0, None)) @ mag, min=1e-5))[0]


def assert_mel_within_frontend_bar(name, got, ref32, audio):
    """The mel bar of tests/test_mel_gpu.py::_check (4 x max and 2 x mean of the reference's own fp32 spread against the float64
    restatement ``mel_helpers.mel_fp64``, + 1e-6 / 1e-7), here with the fixture's ``mel_loss`` as the reference."""
    from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank
    f64, _ = mh.mel_fp64(audio, mel_filter_bank(SR, 1024, 80, 0.0, mh.FMAX['full']))
    spread = np.abs(ref32.astype(np.float64) - f64)
    dm = np.abs(got.astype(np.float64) - f64)
    print(f'{name}: mel max {dm.max():.2e} (ref {spread.max():.2e}) mean {dm.mean():.2e} (ref {spread.mean():.2e})')
    assert dm.max() <= 4 * spread.max() + 1e-6 and dm.mean() <= 2 * spread.mean() + 1e-7, (name, dm.max(), dm.mean(), spread.max(), spread.mean())


# ---- the fine-tuner of the loop tests: the seeded states tests/test_finetune_gpu.py builds its tuners from ----------------------------
@functools.lru_cache(maxsize=None)
def checkpoints():
    from tests import disc_helpers as dh
    from tests import vocoder_helpers
    return {'generator': vocoder_helpers.state_dict('v3')}, dh.state_dicts()


def tuner(device, gen=None, disc=None):
    import ubisoft_laforge_daft_exprt_amd as pkg
    g, d = checkpoints()
    return pkg.HiFiGanFineTuner(g if gen is None else gen, d if disc is None else disc, device)


def parameter_keys(t):
    """The keys of ``tuner_state`` that are parameters (the spectral-norm buffers are state, not parameters)."""
    D = t.discriminators
    return [f'{tag}.{k}' for tag, m in (('g', t.generator), ('mpd', D.mpd), ('msd', D.msd)) for k, _ in m.named_parameters()]


def tuner_state(t):
    """Everything a step changes, on the CPU: parameters and buffers, moments, folded weights; and the counters and learning rates."""
    out = {f'g.{k}': v.detach().cpu().clone() for k, v in t.generator.state_dict().items()}
    out.update((f'mpd.{k}', v.detach().cpu().clone()) for k, v in t.discriminators.mpd.state_dict().items())
    out.update((f'msd.{k}', v.detach().cpu().clone()) for k, v in t.discriminators.msd.state_dict().items())
    for tag, opt in (('og', t.optim_g), ('od', t.optim_d)):
        out.update((f'{tag}.m{i}', m.cpu().clone()) for i, m in enumerate(opt.exp_avg))
        out.update((f'{tag}.s{i}', s.cpu().clone()) for i, s in enumerate(opt.exp_avg_sq))
        out.update((f'{tag}.W.{n}', w.detach().cpu().clone()) for n, w in opt.W.items())
    return out, (t.step, t.epoch, t.optim_g.step_count, t.optim_d.step_count, t.optim_g.lr, t.optim_d.lr)
