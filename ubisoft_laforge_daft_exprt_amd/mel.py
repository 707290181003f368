"""Mel front end on gfx950: waveform -> log-mel spectrogram and frame energy (reference extract_features.py:345-379
``mel_spectrogram_HiFi``, vocoder/dataset.py:26-64 ``mel_spectrogram`` with ``center=False``, extract_features.py:314-319
``extract_energy`` on ``exp(mel)``).

Per utterance of ``len`` samples: reflect-pad by (n_fft - hop) / 2 = 384 with the row's own edge samples, ``len // 256`` frames of
1024 samples under the periodic Hann window, ``mag = sqrt(re^2 + im^2 + 1e-9)``, ``mel = fb @ mag``, ``log(max(mel, min_clipping))``,
energy = L2 norm of ``max(mel, min_clipping)`` over channels.  ``MelSpectrogram`` runs a padded (B, S_max) device batch in one launch
(csrc/dx_mel.hip); row b is bitwise that utterance run alone, and everything at or past a row's frame count is 0.  The filter bank is
``mel_filter_bank``, a restatement of librosa's default ``filters.mel`` (Slaney scale and area normalisation).  There is no CPU path.

The log-mel is differentiable with respect to the waveform: when ``wavs`` requires grad, ``mels`` carries a ``grad_fn`` whose backward
is one ``dx_mel_bwd`` launch (the forward saves only the waveform; the spectrum is recomputed).  ``MelL1Loss`` is the mel term of the
vocoder's generator loss (reference vocoder/finetune_hifigan.py:211-231) on that gradient.  Energy and frame counts carry no gradient.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from ._lib import lib

N_FFT, HOP = 1024, 256
PAD = (N_FFT - HOP) // 2        # 384: reflect padding per side; a row needs more samples than this
DEFAULTS = dict(sampling_rate=22050, filter_length=1024, hop_length=256, n_mel_channels=80, mel_fmin=0.0, mel_fmax=8000.0,
                min_clipping=1e-5)
_FROM_HPARAMS = object()

# Slaney mel scale (librosa.hz_to_mel / mel_to_hz with htk=False): linear below 1 kHz (200/3 Hz per mel), logarithmic above
_F_SP, _MIN_LOG_HZ = 200.0 / 3, 1000.0
_MIN_LOG_MEL, _LOGSTEP = _MIN_LOG_HZ / _F_SP, np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


@functools.lru_cache(maxsize=None)
def _filter_bank(sr, n_fft, n_mels, fmin, fmax):
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.fft.rfftfreq(n=n_fft, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    weights = np.zeros((n_mels, 1 + n_fft // 2), dtype=np.float32)
    for i in range(n_mels):                              # triangles from the ramps, stored in float32 as librosa stores them
        weights[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]     # Slaney area normalisation
    weights.setflags(write=False)
    return weights


def mel_filter_bank(sr, n_fft, n_mels, fmin=0.0, fmax=None) -> np.ndarray:
    """librosa.filters.mel(sr=sr, n_fft=n_fft, n_mels=n_mels, fmin=fmin, fmax=fmax) with its defaults (htk=False, norm='slaney'):
    (n_mels, 1 + n_fft // 2) float32.  ``fmax=None``: sr / 2.  Cached per configuration (a fresh copy is returned)."""
    return _filter_bank(float(sr), int(n_fft), int(n_mels), float(fmin), None if fmax is None else float(fmax)).copy()


def n_frames(length: int) -> int:
    """Frames of an utterance of ``length`` samples: the reflect-padded signal (length + 768) framed by 1024 / 256."""
    return int(length) // HOP


def check_stft(n_fft, win_size, hop_size, center=False):
    if center:
        raise NotImplementedError('the gfx950 mel front end implements center=False (HiFi-GAN framing) only')
    if (int(n_fft), int(win_size), int(hop_size)) != (N_FFT, N_FFT, HOP):
        raise NotImplementedError(f'the gfx950 mel front end implements n_fft = win_size = {N_FFT}, hop = {HOP}; '
                                  f'got n_fft={n_fft}, win_size={win_size}, hop={hop_size}')


def check_lengths(host_lengths, S):
    for b, n in enumerate(host_lengths):
        if n <= PAD:
            raise ValueError(f'row {b}: {n} samples; reflect padding by {PAD} needs more than {PAD} (as torch.nn.functional.pad)')
        if n > S:
            raise ValueError(f'row {b}: length {n} exceeds the {S} samples of the batch')


class MelSpectrogram:
    """Batched log-mel + frame energy on the device.  Configuration from ``hparams`` (any object; missing keys take the reference
    defaults ``DEFAULTS``); ``fmax`` overrides ``hparams.mel_fmax`` (None: full band, as the vocoder's loss mel)."""

    def __init__(self, hparams=None, fmax=_FROM_HPARAMS, device='cuda'):
        hp = lambda k: getattr(hparams, k, DEFAULTS[k]) if hparams is not None else DEFAULTS[k]
        n_fft, hop = int(hp('filter_length')), int(hp('hop_length'))
        check_stft(n_fft, n_fft, hop)
        self.sampling_rate = int(hp('sampling_rate'))
        self.n_mels = int(hp('n_mel_channels'))
        self.fmin = float(hp('mel_fmin'))
        self.fmax = hp('mel_fmax') if fmax is _FROM_HPARAMS else fmax
        self.fmax = None if self.fmax is None else float(self.fmax)
        self.min_clipping = float(hp('min_clipping'))
        if self.n_mels % 16 or self.n_mels > 128:
            raise NotImplementedError(f'n_mel_channels must be a multiple of 16 and at most 128, got {self.n_mels}')
        self.filter_bank = mel_filter_bank(self.sampling_rate, n_fft, self.n_mels, self.fmin, self.fmax)
        nz = np.flatnonzero(self.filter_bank.any(axis=0))
        self.kmax = int(nz[-1]) + 1 if nz.size else 1   # bins at or past kmax have no weight in any channel: never computed
        if self.kmax > N_FFT // 2:
            raise NotImplementedError('a filter bank with weight on the Nyquist bin is not supported')
        self.device = torch.device(device)
        self._ops = None
        self._bwd_ops = None
        self._lengths = {}                              # host lengths -> (int32 lengths, frames) on the device

    def _operands(self):
        if self._ops is None:
            if self.device.type != 'cuda':
                raise RuntimeError('MelSpectrogram runs on the GPU (gfx950 HIP kernel); there is no CPU path')
            nb, nf = torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
            lib().dx_mel_basis_size(self.n_mels, self.kmax, nb.data_ptr(), nf.data_ptr())
            basis = torch.empty(int(nb.item()), dtype=torch.uint8, device=self.device)
            fbp = torch.empty(int(nf.item()), dtype=torch.uint8, device=self.device)
            fb = torch.from_numpy(self.filter_bank).to(self.device).contiguous()
            lib().dx_mel_pack(fb.data_ptr(), self.n_mels, fb.shape[1], self.kmax, basis.data_ptr(), fbp.data_ptr(),
                              torch.cuda.current_stream(self.device).cuda_stream)
            self._ops = (basis, fbp, fb)
        return self._ops

    def _backward_operands(self):
        if self._bwd_ops is None:
            basis, fbp, fb = self._operands()
            basis_t, fb_t = torch.empty_like(basis), torch.empty_like(fbp)      # the transposed packs have the forward packs' sizes
            lib().dx_mel_bwd_pack(fb.data_ptr(), self.n_mels, fb.shape[1], self.kmax, basis_t.data_ptr(), fb_t.data_ptr(),
                                  torch.cuda.current_stream(self.device).cuda_stream)
            self._bwd_ops = (basis_t, fb_t)
        return self._bwd_ops

    def _launch(self, wavs, lens_i32, T):
        B, S = wavs.shape
        basis, fbp, _ = self._operands()
        mels = torch.empty(B, self.n_mels, T, dtype=torch.float32, device=wavs.device)
        energy = torch.empty(B, T, dtype=torch.float32, device=wavs.device)
        lib().dx_mel(wavs.data_ptr(), S, S, lens_i32.data_ptr(), basis.data_ptr(), fbp.data_ptr(), mels.data_ptr(), self.n_mels * T,
                     energy.data_ptr(), B, T, self.n_mels, self.kmax, self.min_clipping, torch.cuda.current_stream(wavs.device).cuda_stream)
        return mels, energy

    def _launch_backward(self, wavs, lens_i32, gmel):
        B, S = wavs.shape
        T = gmel.shape[2]
        basis, fbp, _ = self._operands()
        basis_t, fb_t = self._backward_operands()
        gmel = gmel.float().contiguous()
        dwav = torch.empty_like(wavs)
        lib().dx_mel_bwd(wavs.data_ptr(), S, S, lens_i32.data_ptr(), basis.data_ptr(), fbp.data_ptr(), basis_t.data_ptr(), fb_t.data_ptr(),
                         gmel.data_ptr(), self.n_mels * T, dwav.data_ptr(), B, T, self.n_mels, self.kmax, self.min_clipping,
                         torch.cuda.current_stream(wavs.device).cuda_stream)
        return dwav

    def __call__(self, wavs, lengths):
        """wavs (B, S_max) fp32 on the device; lengths: B sample counts, host ints (no host sync: capturable once the same lengths
        have run eagerly) or a device tensor (one small device-to-host copy sizes the output).  -> (mels (B, n_mels, T_max),
        energy (B, T_max), frames (B,) int64 on the device), T_max = max(lengths) // 256.

        If ``wavs`` requires grad (and grad mode is on), ``mels`` is differentiable once with respect to it: same launch, same bits,
        and a backward of one launch with no host sync (capturable like the forward once a forward and backward have run eagerly).
        ``energy`` and ``frames`` carry no gradient."""
        if wavs.dim() != 2:
            raise ValueError(f'MelSpectrogram: wavs must be (B, S_max), got shape {tuple(wavs.shape)}')
        if wavs.device.type != 'cuda':
            raise ValueError(f'MelSpectrogram: wavs must be on the GPU, got {wavs.device}')
        wavs = wavs.float().contiguous()
        B, S = wavs.shape
        dev = wavs.device
        if torch.is_tensor(lengths):
            host = [int(v) for v in lengths.tolist()]                     # the one device-to-host copy (sizing and checks)
            check_lengths(host, S)
            lens_i32 = lengths.to(device=dev, dtype=torch.int32).contiguous()
            frames = lens_i32.to(torch.long) // HOP
        else:
            host = [int(v) for v in lengths]
            check_lengths(host, S)
            key = (tuple(host), str(dev))
            if key not in self._lengths:
                li = torch.tensor(host, dtype=torch.int32).to(dev)
                self._lengths[key] = (li, li.to(torch.long) // HOP)
            lens_i32, frames = self._lengths[key]
        if len(host) != B:
            raise ValueError(f'MelSpectrogram: {len(host)} lengths for a batch of {B}')
        T = max(n_frames(n) for n in host)
        if wavs.requires_grad and torch.is_grad_enabled():
            mels, energy = _MelFunction.apply(wavs, self, lens_i32, T)
        else:
            mels, energy = self._launch(wavs, lens_i32, T)
        return mels, energy, frames


class _MelFunction(torch.autograd.Function):
    """mels with the waveform gradient of csrc/dx_mel.hip's backward kernel; energy (and the integer frame counts, which never enter
    here) are not differentiable.  Saves the waveform and the lengths only."""

    @staticmethod
    def forward(ctx, wavs, frontend, lens_i32, T):
        mels, energy = frontend._launch(wavs, lens_i32, T)
        frontend._backward_operands()                    # packed now, so that a captured backward launches nothing but the kernel
        ctx.frontend = frontend
        ctx.save_for_backward(wavs, lens_i32)
        ctx.mark_non_differentiable(energy)
        return mels, energy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gmel, _genergy):
        wavs, lens_i32 = ctx.saved_tensors
        return ctx.frontend._launch_backward(wavs, lens_i32, gmel), None, None, None


_FRONTENDS = {}


def _frontend(sr, n_mels, fmin, fmax, clip, device):
    key = (int(sr), int(n_mels), float(fmin), None if fmax is None else float(fmax), float(clip), str(device))
    if key not in _FRONTENDS:
        hp = dict(sampling_rate=sr, filter_length=N_FFT, hop_length=HOP, n_mel_channels=n_mels, mel_fmin=fmin, mel_fmax=fmax,
                  min_clipping=clip)
        _FRONTENDS[key] = MelSpectrogram(type('MelConfig', (), hp)(), device=device)
    return _FRONTENDS[key]


def mel_spectrogram_HiFi(wav, hparams):
    """Drop-in for the reference's extract_features.mel_spectrogram_HiFi: numpy (T,) waveform -> numpy (n_mels, T // 256) log-mel."""
    hp = lambda k: getattr(hparams, k, DEFAULTS[k])
    check_stft(hp('filter_length'), hp('filter_length'), hp('hop_length'))
    fe = _frontend(hp('sampling_rate'), hp('n_mel_channels'), hp('mel_fmin'), hp('mel_fmax'), hp('min_clipping'), 'cuda')
    w = torch.as_tensor(np.asarray(wav, dtype=np.float32)).reshape(1, -1)
    check_lengths([w.shape[1]], w.shape[1])
    mels, _, _ = fe(w.to(fe.device), [w.shape[1]])
    return mels[0].cpu().numpy()


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    """Drop-in for the reference's vocoder/dataset.mel_spectrogram: (B, S) waveforms -> (B, num_mels, S // 256) log-mel (clip 1e-5),
    on the GPU; the result is on ``y``'s device.  Differentiable with respect to ``y`` as ``MelSpectrogram`` is, so the reference's
    ``F.l1_loss(y_mel, mel_spectrogram(y_g_hat.squeeze(1), ...))`` back-propagates into the generated waveform."""
    check_stft(n_fft, win_size, hop_size, center)
    y2 = y.reshape(1, -1) if y.dim() == 1 else y
    check_lengths([y2.shape[1]], y2.shape[1])
    dev = y.device if y.device.type == 'cuda' else torch.device('cuda')
    fe = _frontend(sampling_rate, num_mels, fmin, fmax, 1e-5, dev)
    mels, _, _ = fe(y2.to(dev), [y2.shape[1]] * y2.shape[0])
    return mels.to(y.device)


class MelL1Loss:
    """The mel term of the vocoder's generator loss (reference vocoder/finetune_hifigan.py:211-231, ``F.l1_loss(y_mel, y_g_hat_mel) *
    45`` on the full-band mel): ``scale * sum_valid |mel(wav_hat) - target_mel| / (n_mels * sum_b frames[b])``, differentiable with
    respect to ``wav_hat`` through the HIP backward.  With equal lengths this is the reference's mean over the whole tensor.  With
    ragged lengths the cells at or past a row's frame count are left out of both the sum and the count (they are padding in both
    mels, and whatever ``target_mel`` holds there is ignored), so a short row weighs by its own frames only."""

    def __init__(self, fmax=None, scale=45.0, device='cuda'):
        self.frontend = MelSpectrogram(fmax=fmax, device=device)
        self.scale = float(scale)

    def __call__(self, wav_hat, lengths, target_mel):
        """wav_hat (B, S_max), lengths as for ``MelSpectrogram``, target_mel (B, n_mels, >= T_max) log-mel -> scalar."""
        mels, _, frames = self.frontend(wav_hat, lengths)
        T = mels.shape[2]
        if target_mel.dim() != 3 or target_mel.shape[0] != mels.shape[0] or target_mel.shape[1] != mels.shape[1] or target_mel.shape[2] < T:
            raise ValueError(f'MelL1Loss: target_mel {tuple(target_mel.shape)} does not cover the mel {tuple(mels.shape)}')
        keep = (torch.arange(T, device=mels.device)[None, :] < frames[:, None])[:, None, :]
        delta = mels - target_mel[:, :, :T].to(mels.dtype)
        total = torch.where(keep, delta, torch.zeros((), dtype=delta.dtype, device=delta.device)).abs().sum()   # masked before abs: no NaN leaks back
        return total * self.scale / (frames.sum() * mels.shape[1])
