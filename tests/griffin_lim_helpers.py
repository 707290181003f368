"""Restatements of the Griffin-Lim path for the tests, written from the algorithm's description (not from the reference's code):
the iteration vectorised over frames in float64 or float32 (``scipy.fft`` keeps single precision), the spectral convergence, the
NNLS residual, a float32 FISTA, and the unpacking of the two packed forms of the filter bank."""
import os

import numpy as np
import scipy.fft

N_FFT, HOP, N_BINS = 1024, 256, 513
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'griffin_lim.npz')
ITERS = (1, 8, 32)
STARTS = ('noise', 'zeros')


def golden():
    with np.load(GOLDEN) as d:
        return {k: d[k] for k in d.files}


def _frame_index(T):
    return HOP * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]


def stft(x, T, dtype=np.float64):
    """x (256 T + 1024,) -> (T, 513) spectra of the frames at 256 i under the symmetric Hann window."""
    w = np.hanning(N_FFT).astype(dtype)
    return scipy.fft.rfft(w * np.asarray(x, dtype=dtype)[_frame_index(T)], axis=1)


def gl_step(M, x, dtype=np.float64):
    """One iteration: M (513, T) magnitudes, x (256 T + 1024,) -> the next x.  Phase of a zero bin: (1, 0); the synthesis takes DC and
    Nyquist as real (c2r transforms ignore their imaginary parts); a block's up-to-four frames are added in frame order."""
    T = M.shape[1]
    w = np.hanning(N_FFT).astype(dtype)
    S = stft(x, T, dtype)
    mag = np.abs(S)
    unit = np.where(mag == 0, 1.0, S / np.where(mag == 0, 1.0, mag))
    P = (np.asarray(M, dtype=dtype).T * unit).astype(S.dtype)
    y = (w * scipy.fft.irfft(P, n=N_FFT, axis=1)).reshape(T, 4, HOP)
    out = np.zeros((T + 4, HOP), dtype=dtype)
    for d in (3, 2, 1, 0):                                   # block s takes frame s - d's segment d: oldest frame first
        out[d:d + T] += y[:, d]
    return (out.reshape(-1) / dtype(2)).astype(dtype)


def gl_iterate(M, x0, iterations, dtype=np.float64, keep=()):
    """-> x after ``iterations`` steps (and {k: x after k steps} for k in ``keep``)."""
    x = np.asarray(x0, dtype=dtype)
    kept = {}
    for k in range(1, iterations + 1):
        x = gl_step(M, x, dtype)
        if k in keep:
            kept[k] = x
    return (x, kept) if keep else x


def spectral_convergence(x, M):
    """| |STFT(x)| - M |_F / |M|_F in float64."""
    M = np.asarray(M, dtype=np.float64)
    return float(np.linalg.norm(np.abs(stft(x, M.shape[1])).T - M) / np.linalg.norm(M))


def relative_residual(A, X, m):
    """|A X - m|_F / |m|_F in float64."""
    A, X, m = (np.asarray(v, dtype=np.float64) for v in (A, X, m))
    return float(np.linalg.norm(A @ X - m) / np.linalg.norm(m))


def fista32(A, m, steps=200):
    """Float32 FISTA on 1/2 |A x - m|^2, x >= 0, from max(pinv(A) m, 0) with step 1 / |A|_2^2 (both from double, rounded once)."""
    A64 = np.asarray(A, dtype=np.float32).astype(np.float64)
    A32 = A64.astype(np.float32)
    pinv = np.linalg.pinv(A64).astype(np.float32)
    step = np.float32(1.0 / np.linalg.norm(A64, 2) ** 2)
    m = np.asarray(m, dtype=np.float32)
    x = np.maximum(pinv @ m, np.float32(0))
    y, t = x.copy(), np.float32(1)
    for _ in range(steps):
        g = A32.T @ (A32 @ y - m)
        xn = np.maximum(y - step * g, np.float32(0))
        tn = np.float32(0.5) * (np.float32(1) + np.sqrt(np.float32(1) + np.float32(4) * t * t))
        y = xn + ((t - np.float32(1)) / tn) * (xn - x)
        x, t = xn, tn
    assert x.dtype == np.float32
    return x


def unpack_bins(pack, n_mels, KP=576):
    """The per-bin form of the packed bank (two channel indices, two weights) -> dense (n_mels, 513)."""
    A = np.zeros((n_mels, N_BINS), dtype=np.float32)
    w = pack[KP:3 * KP].view(np.float32).reshape(2, KP)
    for k in range(N_BINS):
        i0, i1 = int(pack[k]) & 0xFFFF, (int(pack[k]) >> 16) & 0xFFFF
        A[i0, k] += w[0, k]
        A[i1, k] += w[1, k]
    return A


def unpack_channels(pack, n_mels, KP=576, MAXCH=128):
    """The per-channel form (first bin, count, offset, channel-major weights) -> dense (n_mels, 513)."""
    A = np.zeros((n_mels, N_BINS), dtype=np.float32)
    base = 3 * KP
    chw = pack[base + 3 * MAXCH:].view(np.float32)
    for n in range(n_mels):
        lo, cnt, off = (int(pack[base + i * MAXCH + n]) for i in range(3))
        A[n, lo:lo + cnt] = chw[off:off + cnt]
    return A
