"""Griffin-Lim on gfx950: mel -> waveform with no vocoder checkpoint (reference griffin_lim.py:100-198, the vocoding of
``synthesize.py --use_griffin_lim``).

Per utterance the reference computes ``m = exp(mel)`` (80, T); ``X = nnls(A, m)`` (513, T), ``A`` the mel filter bank; Griffin-Lim on
``X[:, :-2]`` -- the last two frames are dropped -- and ``x / max|x|``.  With T' = T - 2 frames the signal has 256 T' + 1024 samples and
every iteration analyses the T' frames starting at samples 256 i under the symmetric Hann window ``np.hanning(1024)``:
``S_i = rfft(w x_i)``, ``P_i = M_i exp(j angle(S_i))``, ``x <- overlap_add(w irfft(P_i)) / 2``.  Here a padded batch runs one launch per
iteration (csrc/dx_griffin_lim.hip: a 1024-point radix-4 FFT in LDS, two frames per complex transform, atomics-free overlap-add), the
launches captured once per (B, T_max, iterations) as a linear graph; the non-negative least squares is a fixed number of FISTA steps,
one wave per frame.  fp32 throughout; there is no CPU path.

What is and is not pinned.  ``mel_to_linear`` is underdetermined (80 equations, 513 unknowns): the reference's answer depends on
L-BFGS-B's path and is one minimiser among many, so neither ``X`` nor the audio made from a mel reproduces the reference's; the residual
``|A X - m| / |m|`` does (it is smaller here).  Griffin-Lim itself is pinned from a given magnitude and a given start signal.

Deviations from the reference, both so that one row cannot kill a batch: a row with fewer than 3 mel frames (no frame left after the
drop) comes back silent with sample length 0 where the reference raises, and an all-zero signal stays zero under the peak
normalisation where the reference divides by zero (NaN).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import lib
from .graphs import Entry, GraphCache, capture
from .mel import DEFAULTS, HOP, N_FFT, mel_filter_bank

N_BINS = N_FFT // 2 + 1
KP, MAX_CHANNELS, CHANNEL_WEIGHTS = 576, 128, 1536      # dx_nnls_mel's pack: padded bins, channel slots, channel-major weight slots
PACK_WORDS = 3 * KP + 3 * MAX_CHANNELS + CHANNEL_WEIGHTS
_PASSES = (4, 16, 64, 256)


def check_geometry(n_fft, hop):
    if (int(n_fft), int(hop)) != (N_FFT, HOP):
        raise NotImplementedError(f'Griffin-Lim on gfx950 implements filter_length = win = {N_FFT}, hop = {HOP}; '
                                  f'got filter_length={n_fft}, hop={hop}')


def gl_tables() -> np.ndarray:
    """The 3072 floats dx_gl_iter reads, computed in double and rounded once: ``np.hanning(1024)``, then the cos and -sin twiddles of
    the radix-4 passes Ns = 4, 16, 64, 256 at offset Ns - 4, laid out [r - 1][q] for the angle 2 pi q r / (4 Ns)."""
    tab = np.zeros(3 * N_FFT, dtype=np.float64)
    tab[:N_FFT] = np.hanning(N_FFT)
    for ns in _PASSES:
        q = np.arange(ns, dtype=np.float64)
        for r in (1, 2, 3):
            ang = 2.0 * np.pi * q * r / (4 * ns)
            o = ns - 4 + (r - 1) * ns
            tab[N_FFT + o:N_FFT + o + ns] = np.cos(ang)
            tab[2 * N_FFT + o:2 * N_FFT + o + ns] = -np.sin(ang)
    return tab.astype(np.float32)


def pack_filter_bank(bank):
    """(n_mels, 513) filter bank -> dict(pack int32 (PACK_WORDS,), pinv_t float32 (n_mels, 576), step float): the operands of
    dx_nnls_mel.  The kernel relies on the triangular structure, which is validated here: every frequency bin has at most two non-zero
    weights, and each channel's non-zeros are one run of consecutive bins.  Any other bank raises ValueError.  ``pinv(A)`` and the
    FISTA step ``1 / |A|_2^2`` are computed in double and rounded once."""
    A = np.asarray(bank)
    if A.ndim != 2 or A.shape[1] != N_BINS or not 0 < A.shape[0] <= MAX_CHANNELS:
        raise ValueError(f'filter bank must be (n_mels <= {MAX_CHANNELS}, {N_BINS}), got {A.shape}')
    A32 = A.astype(np.float32)
    n_mels = A32.shape[0]
    nz = A32 != 0
    per_bin = nz.sum(axis=0)
    if per_bin.max() > 2:
        k = int(np.argmax(per_bin))
        raise ValueError(f'filter bank: bin {k} has {int(per_bin[k])} non-zero weights; the kernel takes at most two per bin')
    words = np.zeros(PACK_WORDS, dtype=np.int32)
    w = np.zeros((2, KP), dtype=np.float32)
    for k in range(N_BINS):
        ch = np.flatnonzero(nz[:, k])
        i0 = int(ch[0]) if ch.size > 0 else 0
        i1 = int(ch[1]) if ch.size > 1 else i0
        words[k] = i0 | (i1 << 16)
        if ch.size > 0:
            w[0, k] = A32[i0, k]
        if ch.size > 1:
            w[1, k] = A32[i1, k]
    words[KP:3 * KP] = w.reshape(-1).view(np.int32)
    chw = np.zeros(CHANNEL_WEIGHTS, dtype=np.float32)
    off = 0
    for n in range(n_mels):
        ks = np.flatnonzero(nz[n])
        lo, cnt = (int(ks[0]), int(ks.size)) if ks.size else (0, 0)
        if cnt and int(ks[-1]) - lo + 1 != cnt:
            raise ValueError(f'filter bank: the non-zero weights of channel {n} are not one run of consecutive bins')
        words[3 * KP + n], words[3 * KP + MAX_CHANNELS + n], words[3 * KP + 2 * MAX_CHANNELS + n] = lo, cnt, off
        chw[off:off + cnt] = A32[n, lo:lo + cnt]
        off += cnt
    words[3 * KP + 3 * MAX_CHANNELS:] = chw.view(np.int32)
    A64 = A32.astype(np.float64)
    pinv_t = np.zeros((n_mels, KP), dtype=np.float32)
    pinv_t[:, :N_BINS] = np.linalg.pinv(A64).T
    step = 1.0 / np.linalg.norm(A64, 2) ** 2
    return dict(pack=words, pinv_t=pinv_t, step=float(step))


def layout():
    """-> (hop blocks one workgroup of dx_gl_iter owns, 32-bit words of dx_nnls_mel's packed bank), as the library states them."""
    import ctypes
    tile, words = ctypes.c_int(0), ctypes.c_int(0)
    lib().dx_gl_layout(ctypes.addressof(tile), ctypes.addressof(words))
    return tile.value, words.value


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class GriffinLim:
    """Batched mel -> waveform on the device.  Configuration from ``hparams`` (any object; missing keys take the reference defaults of
    ``mel.DEFAULTS``).  ``iterations``: Griffin-Lim passes (the reference runs 500); ``nnls_iterations``: FISTA steps of the mel ->
    linear solve.  Only ``filter_length = 1024`` and ``hop_length = 256`` are implemented; anything else raises NotImplementedError."""

    MAX_GRAPHS = 8

    def __init__(self, hparams=None, iterations=500, nnls_iterations=200, device='cuda'):
        hp = lambda k: getattr(hparams, k, DEFAULTS[k]) if hparams is not None else DEFAULTS[k]
        check_geometry(hp('filter_length'), hp('hop_length'))
        if int(iterations) < 0 or int(nnls_iterations) < 0:
            raise ValueError('GriffinLim: iterations and nnls_iterations must not be negative')
        self.iterations, self.nnls_iterations = int(iterations), int(nnls_iterations)
        self.n_mels = int(hp('n_mel_channels'))
        fmax = hp('mel_fmax')
        self.filter_bank = mel_filter_bank(int(hp('sampling_rate')), N_FFT, self.n_mels, float(hp('mel_fmin')),
                                           None if fmax is None else float(fmax))
        self.bank = pack_filter_bank(self.filter_bank)           # raises for a bank the kernel cannot take
        self.device = torch.device(device)
        self._ops = None
        self._graphs = GraphCache(self.MAX_GRAPHS, 'oldest')     # (B, T, iterations) -> captured chain and its static buffers
        self.captures = 0

    # -- operands ----------------------------------------------------------------------------------------------------------------
    def _operands(self):
        if self._ops is None:
            if self.device.type != 'cuda':
                raise RuntimeError('GriffinLim runs on the GPU (gfx950 HIP kernels); there is no CPU path')
            assert layout()[1] == PACK_WORDS
            dev = lambda a: torch.from_numpy(a).to(self.device).contiguous()
            self._ops = dict(tab=dev(gl_tables()), pack=dev(self.bank['pack']), pinv_t=dev(self.bank['pinv_t']))
        return self._ops

    def _frames(self, lengths, B, T, dev, who):
        """-> int32 frame counts on the device, clamped to [0, T]."""
        if torch.is_tensor(lengths):
            frames = lengths.to(device=dev, dtype=torch.int32)
        else:
            frames = torch.tensor([int(v) for v in lengths], dtype=torch.int32).to(dev)
        if frames.shape != (B,):
            raise ValueError(f'{who}: {tuple(frames.shape)} lengths for a batch of {B}')
        return frames.clamp(0, T).contiguous()

    def _check(self, who, t, channels):
        if t.dim() != 3 or t.shape[1] != channels or t.shape[0] < 1:
            raise ValueError(f'{who}: expected (B, {channels}, T), got {tuple(t.shape)}')
        if t.device.type != 'cuda':
            raise RuntimeError(f'{who} runs on the GPU (gfx950 HIP kernels); there is no CPU path')

    # -- mel -> linear -----------------------------------------------------------------------------------------------------------
    def mel_to_linear(self, mels, lengths, nnls_iterations=None):
        """mels (B, n_mels, T) LINEAR-scale (``exp`` of the log-mel) fp32 on the device, lengths: B frame counts -> X (B, 513, T), X >= 0
        with ``|A X - mels|`` minimised per frame by ``nnls_iterations`` FISTA steps from ``max(pinv(A) mels, 0)``; frames at or past a
        row's length are 0 and row b is bitwise that utterance alone.  The result is a (B, 513, T) view of frame-major storage, the
        layout ``reconstruct`` reads.  The minimiser is not unique and is not the reference's (see the module docstring)."""
        self._check('mel_to_linear', mels, self.n_mels)
        mels = mels.float().contiguous()
        B, _, T = mels.shape
        dev = mels.device
        out = torch.empty(B, max(T, 1), N_BINS, dtype=torch.float32, device=dev)[:, :T]
        if T == 0:
            return out.transpose(1, 2)
        frames = self._frames(lengths, B, T, dev, 'mel_to_linear')
        ops = self._operands()
        iters = self.nnls_iterations if nnls_iterations is None else int(nnls_iterations)
        lib().dx_nnls_mel(mels.data_ptr(), self.n_mels * T, frames.data_ptr(), ops['pinv_t'].data_ptr(), ops['pack'].data_ptr(),
                          self.bank['step'], iters, out.data_ptr(), T * N_BINS, B, T, self.n_mels, N_BINS, _stream(dev))
        return out.transpose(1, 2)

    # -- the iteration -----------------------------------------------------------------------------------------------------------
    def _chain(self, xa, xb, mag, smb, frames, B, T, iterations, dev):
        tab, st = self._operands()['tab'], _stream(dev)
        S = xa.shape[1]
        src, dst = xa, xb
        for _ in range(iterations):
            lib().dx_gl_iter(src.data_ptr(), dst.data_ptr(), S, mag.data_ptr(), smb, frames.data_ptr(), tab.data_ptr(), B, T, N_FFT, HOP, st)
            src, dst = dst, src
        return src

    def reconstruct(self, magnitudes, lengths, init=None, generator=None, iterations=None, use_graph=True):
        """magnitudes (B, 513, T) fp32 on the device, lengths: B frame counts -> (x (B, 256 T + 1024), sample_lengths (B,) int64 on the
        device): ``iterations`` Griffin-Lim passes from ``init`` (B, 256 T + 1024), or from ``torch.randn`` on the device drawn from
        ``generator``.  Row b uses its own ``lengths[b]`` frames, has 256 lengths[b] + 1024 samples (0 for a row of no frames) and zeros
        past them, and is bitwise that utterance alone from the same start signal.  With ``use_graph`` the chain of launches is captured
        once per (B, T, iterations) and replayed (bitwise the eager result)."""
        self._check('reconstruct', magnitudes, N_BINS)
        B, _, T = magnitudes.shape
        dev = magnitudes.device
        iterations = self.iterations if iterations is None else int(iterations)
        if iterations < 0:
            raise ValueError('reconstruct: iterations must not be negative')
        S = HOP * T + N_FFT
        frames = self._frames(lengths, B, T, dev, 'reconstruct')
        frames64 = frames.to(torch.long)
        sample_lengths = torch.where(frames64 > 0, frames64 * HOP + N_FFT, torch.zeros_like(frames64))
        if init is None:
            init = torch.randn(B, S, dtype=torch.float32, device=dev, generator=generator)
        elif tuple(init.shape) != (B, S):
            raise ValueError(f'reconstruct: init must be ({B}, {S}), got {tuple(init.shape)}')
        init = init.to(device=dev, dtype=torch.float32)
        if T == 0 or iterations == 0:
            keep = torch.arange(S, device=dev)[None, :] < sample_lengths[:, None]
            return torch.where(keep, init, torch.zeros((), dtype=torch.float32, device=dev)), sample_lengths
        mag = magnitudes.float().transpose(1, 2)                          # frame-major: (B, T, 513)
        if mag.stride(2) != 1 or mag.stride(1) != N_BINS or (B > 1 and mag.stride(0) < T * N_BINS):
            mag = mag.contiguous()                                        # the one repack, outside the loop
        smb = mag.stride(0) if B > 1 else T * N_BINS
        if not use_graph:
            xa, xb = init.clone(), torch.empty_like(init)
            return self._chain(xa, xb, mag, smb, frames, B, T, iterations, dev), sample_lengths
        key = (B, T, iterations, str(dev))
        g = self._graphs.get(key)
        if g is None:
            xa, xb = torch.zeros(B, S, dtype=torch.float32, device=dev), torch.zeros(B, S, dtype=torch.float32, device=dev)
            mag_s, frames_s = torch.zeros(B, T, N_BINS, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            chain = lambda n: self._chain(xa, xb, mag_s, T * N_BINS, frames_s, B, T, n, dev)
            chain(1)                                                      # eager warm-up on the current stream: configures the kernel
            torch.cuda.synchronize(dev)
            graph, out = capture(lambda: chain(iterations))
            self.captures += 1
            g = self._graphs[key] = Entry([graph], xa=xa, xb=xb, mag=mag_s, frames=frames_s, out=out)
        g.xa.copy_(init)
        g.mag.copy_(mag)
        g.frames.copy_(frames)
        g.graphs[0].replay()
        return g.out.clone(), sample_lengths

    def peak_normalize(self, x):
        """x (B, S) fp32 on the device -> x / max|x| per row (griffin_lim.py:196).  An all-zero row stays zero; the reference would
        produce NaN there."""
        if x.dim() != 2 or x.device.type != 'cuda':
            raise ValueError(f'peak_normalize: x must be (B, S) on the GPU, got {tuple(x.shape)} on {x.device}')
        x = x.float().contiguous()
        y = torch.empty_like(x)
        B, S = x.shape
        if B and S:
            lib().dx_gl_peak_normalize(x.data_ptr(), y.data_ptr(), S, B, S, _stream(x.device))
        return y

    # -- the whole reference function, batched -----------------------------------------------------------------------------------
    def from_mel(self, log_mels, lengths, init=None, generator=None, iterations=None, nnls_iterations=None, use_graph=True):
        """``griffin_lim_reconstruction_from_mel_spec`` for a padded batch: log_mels (B, n_mels, T) on the device, lengths: B frame counts
        -> (audio (B, 256 (T - 2) + 1024) = (B, 256 T + 512), sample_lengths (B,) int64 on the device).  exp, NNLS, each row's own last
        two frames dropped, Griffin-Lim from ``init`` (B, 256 T + 512) or device noise, peak normalisation.  A row of fewer than 3
        frames comes back silent with sample length 0 (the reference raises there: a batch must not die on one short row)."""
        self._check('from_mel', log_mels, self.n_mels)
        B, _, T = log_mels.shape
        dev = log_mels.device
        Tg = max(T - 2, 0)
        if Tg == 0:
            return torch.zeros(B, N_FFT, dtype=torch.float32, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
        frames = self._frames(lengths, B, T, dev, 'from_mel')
        X = self.mel_to_linear(torch.exp(log_mels.float()), frames, nnls_iterations)
        x, sample_lengths = self.reconstruct(X[:, :, :Tg], (frames - 2).clamp(min=0), init, generator, iterations, use_graph)
        return self.peak_normalize(x), sample_lengths


_INSTANCES = {}


def _instance(hparams, device):
    hp = lambda k: getattr(hparams, k, DEFAULTS[k])
    key = tuple(hp(k) for k in ('sampling_rate', 'filter_length', 'hop_length', 'n_mel_channels', 'mel_fmin', 'mel_fmax')) + (str(device),)
    if key not in _INSTANCES:
        _INSTANCES[key] = GriffinLim(hparams, device=device)
    return _INSTANCES[key]


def griffin_lim_reconstruction_from_mel_spec(mel_spec, hparams, logger=None, *, iterations=500, init=None, generator=None, device='cuda'):
    """Drop-in for the reference's griffin_lim.griffin_lim_reconstruction_from_mel_spec: numpy (n_mels, T) log-mel of ONE utterance ->
    numpy waveform of 256 (T - 2) + 1024 samples, peak-normalised, computed on the GPU (``logger`` is accepted and unused).  The keyword
    arguments are extensions: ``init`` (the start signal in place of device noise), ``generator``, ``iterations``.  T < 3: an empty
    array (the reference raises)."""
    gl = _instance(hparams, device)
    mel = torch.as_tensor(np.asarray(mel_spec, dtype=np.float32))
    if mel.dim() != 2:
        raise ValueError(f'griffin_lim_reconstruction_from_mel_spec takes one (n_mels, T) mel, got shape {tuple(mel.shape)}')
    T = mel.shape[1]
    if init is not None:
        init = torch.as_tensor(np.asarray(init, dtype=np.float32)).reshape(1, -1).to(gl.device)
    audio, lens = gl.from_mel(mel[None].to(gl.device), [T], init=init, generator=generator, iterations=iterations)
    return audio[0, :int(lens[0].item())].cpu().numpy()


class GriffinLimVocoder:
    """The vocoder interface of ``SpeechSynthesizer`` on Griffin-Lim: no checkpoint, no weights.  ``generator``: the torch generator
    the start noise is drawn from on the device (None: the default one)."""

    def __init__(self, hparams=None, iterations=500, nnls_iterations=200, device='cuda', generator=None, use_graph=True):
        self.griffin_lim = GriffinLim(hparams, iterations, nnls_iterations, device)
        self.device = self.griffin_lim.device
        self.generator = generator
        self.use_graph = use_graph

    def infer_batch(self, mels, lengths):
        """mels (B, n_mels, T_max) log-mel on the device, lengths: B frame counts -> (audio (B, 256 T_max + 512) fp32 on the device,
        sample_lengths (B,) int64 on the device: 256 lengths[b] + 512, 0 for a row of fewer than 3 frames)."""
        with torch.no_grad():
            return self.griffin_lim.from_mel(mels, lengths, generator=self.generator, use_graph=self.use_graph)

    def infer(self, mel_spec):
        """(n_mels, T) or (1, n_mels, T) log-mel (numpy, tensor or nested list) -> numpy waveform of 256 T + 512 samples in [-1, 1]."""
        mel = mel_spec.detach().float() if torch.is_tensor(mel_spec) else torch.as_tensor(np.asarray(mel_spec, dtype=np.float32))
        if mel.dim() == 3:
            if mel.shape[0] != 1:
                raise ValueError(f'infer vocodes one utterance, got a batch of {mel.shape[0]} mels: use infer_batch')
            mel = mel[0]
        if mel.dim() != 2:
            raise ValueError(f'infer takes a (n_mels, T) or (1, n_mels, T) mel, got shape {tuple(mel.shape)}')
        audio, lens = self.infer_batch(mel[None].to(self.device), [mel.shape[1]])
        return audio[0, :int(lens[0].item())].cpu().numpy()
