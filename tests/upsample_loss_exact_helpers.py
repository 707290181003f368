"""Float64 restatements of the Gaussian upsampler (csrc/dx_upsample.hip), the loss kernels (csrc/dx_loss.hip) and dx_cross_entropy, the
inputs of their test cases, the a-priori error bounds and the comparison functions (tests/test_upsample_loss_exact_cpu.py tests this
file without a GPU; tests/test_upsample_loss_exact_gpu.py uses it on the C entries).  Everything here runs on the CPU.

Every restatement takes the fp32 buffers its kernel takes and a ``dtype``: float64 is the reference, float32 is the plain fp32 torch
form of the same formula (the CPU file shows that it passes every bound here, so the bounds are attainable by fp32 arithmetic).  The
later stages read buffers an earlier stage wrote (weights, z, dsigma, ep, des): both sides are handed the same fp32 buffer, so the only
difference left is the stage's own rounding.

Bounds.  u = 2^-24.  A value that is a sum of terms, each passing through at most n fp32 additions, errs by at most
(n + 2) u sum|terms| (the project's a-priori form; the sum of magnitudes comes from the float64 restatement).  Factors that are
themselves rounded before they enter the sum add their relative errors to n.  The chain lengths n, with the kernel line they are read
from (csrc/dx_upsample.hip, csrc/dx_loss.hip):

  xs            8: three 3-tap sums with their bias (3 + 3 additions), then (enc + ev) + pv                     (upsample_prep_kernel, `xv[k] = ...`)
  z             13: dv (3), xv + dv (1), two channels per lane (2), dx_wave_sum (6), + br (1)                   (`dot += ...`, `dx_wave_sum(dot) + br`)
  sigma         relative 8 u: expf and log1pf of the fp32 z, both sides branch on the same z                     (`softplus_ref`)
  weights       E = d^2 / (2 sigma^2) + |log sigma| + 0.92; p errs by (8 E + 4) u relatively (the exponent's absolute error is the
                relative error of p); the denominator by the p-weighted mean of that plus (L + 2) u (L / LG strided additions, then
                LG); |dw| <= w (rel_p + rel_den + 2 u) + 1.2e-38 / den (a flushed subnormal p)                  (upsample_fwd_kernel, pass 1)
  x_up          sum_l bound_w |xs| + (2 nk + 1 + 2) u sum_l w |xs|, nk = ceil(len / 4) rounded up to even: two accumulator chains of
                nk / 2 MFMAs of 4 products each, then one addition                                             (upsample_fwd_kernel, pass 2)
  dxs           TT + tiles + 1: TT products on one accumulator, one atomic per frame tile, onto the base        (upsample_bwd_kernel, last loop)
  dsigma        65 + ceil(L / LG) + LG + TT + tiles + 1, LG = 256 / TT: the 128-deep product dw on two accumulators (4 up_mma4 calls
                of 4 MFMAs of 4 products each: 64 products on a chain, then `acc += acc1`), the strided and the final sum of
                `inner`, the thread's loop over the tile's frames, one atomic per frame tile, onto the base; + 8 for the rounded factors
                of (d^2 / sigma^3 - 1 / sigma) w.  sum|terms| is the fully expanded one:
                sum_t w (d^2 / sigma^3 + 1 / sigma) (A[l,t] + sum_l' w[l',t] A[l',t]), A = sum_c |xs g|        (upsample_bwd_kernel, `s += dlp * ...`)
  dz            relative 8 u (expf, 1 + e, the division, the product); the gate at softplus(z) = 1e-3 is ambiguous within 4 ulp of z
  dwr, dbr      4 + rows per wave + 2 + blocks: dv and xv + dv (4), the wave's rows, the four waves (2), one atomic per block
                                                                                                                (upsample_sym_bwd_kernel, `gwr[k] += ...`)
  dxs_out       3 u (|dxs_in| + |dz wr|)
  ep, et        ceil(M / 4) + 2, + 8 for expf squared (the square root halves it; not claimed)                  (mel_stats_kernel, `sp += e1 * e1`)
  l1sum, l2sum  ceil(M / 4) + 6 + 2 + ceil(T / 64): the thread's bins, dx_wave_sum, the four waves, one atomic per 64-frame block;
                + 2 more for l2 (the square of a rounded difference)                                            (mel_stats_kernel, block_sum_256)
  des           diff errs by 9 u (sum_win |ep| + sum_win |et|) / 5: five additions, the division, the subtraction  (energy_diff_kernel)
  esum          sum (2 |diff| eps + eps^2) + (6 + 2 + blocks + 2) u sum diff^2, blocks = B ceil(T / 256) atomics on ONE address
  dmel          8 u (|l1 term| + |l2 term|) + 14 u |energy term| with the pooled |des| in it                    (mel_grad_kernel)
  pitch sums    6 + 2 + B ceil(T / 256), + 2 for the squared difference; the count is an integer below 2^24: exact
  pitch grad    relative 6 u
  finalize      per term ceil(B / 256) + 8 (the thread's loop, block_sum_256) + 6 for the divisions and weights; the total adds six terms
  cross entropy eps_lse = (S + 6) u (|max| + |log z|); dlogits errs by p (eps_lse + u |l - lse| + 3 u) + 2 u |p - onehot|, over B
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
D = 128
LOG_SQRT_2PI = 0.91893853320467274178
F32_TINY = 1.2e-38
DEN_MIN = 2.0 ** -60                 # frames whose float64 denominator is below this are not compared (both sides underflow)
LDS_BUDGET = 150 * 1024
SIGMA_MIN = float(np.float32(1e-3))
EPS_COUNT = float(np.float32(1e-5))
SOFTPLUS_T = 20.0
Z_GATE = math.log(math.expm1(SIGMA_MIN))     # softplus(Z_GATE) = 1e-3f: below it the clamp holds sigma and stops the gradient
PREP_MAX_BLOCKS = 4096
SYM_BWD_BLOCKS = 256
MEL_TT = 64
MAX_EXCLUDED = 0.01


def f32(x):
    """a python float as the C entry receives it"""
    return float(np.float32(x))


def cpu(t, dtype=None):
    t = t.detach().cpu()
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the LDS formulas of dx_upsample.hip, restated
# ---------------------------------------------------------------------------------------------------------------------------------------
def fwd_smem(L, TT=16):
    return (L * TT + (256 // TT) * TT + 2 * L) * 4


def bwd_smem(L, TT):
    Lp = (L + 15) & ~15
    return (TT * (D + 4) + ((Lp * (TT + 1) + 3) & ~3) + Lp * (TT + 4) + 256 + max(32 * (D + 4), D * (TT + 4))) * 4


def bwd_tile(L):
    """frames per workgroup of dx_upsample_bwd at symbol count L; None: refused"""
    if bwd_smem(L, 32) <= LDS_BUDGET:
        return 32
    return 16 if bwd_smem(L, 16) <= LDS_BUDGET else None


def first_over(fn, limit=1 << 16):
    """the smallest L at which fn(L) exceeds the LDS budget"""
    return next(L for L in range(1, limit) if fn(L) > LDS_BUDGET)


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, bound, mask=None):
    """(largest |got - ref| / bound, its index).  A zero bound demands equality; NaN or a breach of a zero bound gives inf."""
    got, ref = cpu(got, torch.float64), cpu(ref, torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    if mask is not None:
        r = torch.where(mask.expand_as(r), r, torch.zeros_like(r))
    if r.numel() == 0:
        return 0.0, ()
    i = int(r.reshape(-1).argmax())
    return float(r.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(r.shape))) if r.dim() else ()


def bits_equal(a, b):
    a, b = cpu(a).contiguous(), cpu(b).contiguous()
    assert a.dtype == b.dtype == torch.float32 and a.shape == b.shape
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def valid_mask(lens, N):
    return torch.arange(N)[None, :] < torch.as_tensor(lens).long()[:, None]


def dyadic(g, shape, span, den):
    """integers in [-span, span] over den (a power of two)"""
    return torch.randint(-span, span + 1, shape, generator=g).float() / den


# ---------------------------------------------------------------------------------------------------------------------------------------
# duration scan
# ---------------------------------------------------------------------------------------------------------------------------------------
SCAN_LENGTHS = (1, 63, 64, 65, 130)


def scan_inputs(L):
    """(3, L) int64: a row of small durations with zeros, a row whose total passes 2^24, a row of zeros with one late nonzero"""
    g = torch.Generator().manual_seed(100 + L)
    d = torch.zeros(3, L, dtype=torch.int64)
    d[0] = torch.randint(0, 13, (L,), generator=g) * (torch.rand(L, generator=g) > 0.3)
    d[1] = torch.randint(0, 2 ** 20, (L,), generator=g)
    d[1, 0] = 2 ** 24 + 3
    d[2, L - 1] = 5
    return d


def scan_ref(dur_int, lost_carry=False):
    """mu (float32: float32(d) / 2 + float32(exclusive cumsum), one fp32 addition) and totals (int64).  ``lost_carry`` (a planted
    error): the prefix restarts at every 64-lane chunk."""
    d = np.asarray(cpu(dur_int), dtype=np.int64)
    incl = np.cumsum(d, axis=1)
    excl = incl - d
    if lost_carry:
        for base in range(64, d.shape[1], 64):
            excl[:, base:base + 64] -= incl[:, base - 1:base]
    mu = d.astype(np.float32) / np.float32(2) + excl.astype(np.float32)
    assert mu.dtype == np.float32
    return torch.from_numpy(mu), torch.from_numpy(incl[:, -1].copy())


# ---------------------------------------------------------------------------------------------------------------------------------------
# prep: xs, z, sigma
# ---------------------------------------------------------------------------------------------------------------------------------------
def _taps(s):
    p = F.pad(s, (1, 1))
    return p[:, :-2, None], p[:, 1:-1, None], p[:, 2:, None]


def conv3(s, w, b, dtype):
    """Conv1d(1 -> D, k = 3, 'same') of s (B, L) -> (B, L, D): b + (w0 s[l-1] + w1 s[l] + w2 s[l+1])"""
    w = cpu(w, dtype).reshape(D, 3)
    s0, s1, s2 = _taps(cpu(s, dtype))
    return cpu(b, dtype) + (s0 * w[:, 0] + s1 * w[:, 1] + s2 * w[:, 2])


def conv3_mag(s, w, b):
    w = cpu(w, torch.float64).reshape(D, 3).abs()
    s0, s1, s2 = _taps(cpu(s, torch.float64).abs())
    return cpu(b, torch.float64).abs() + s0 * w[:, 0] + s1 * w[:, 1] + s2 * w[:, 2]


def prep_inputs(B, L, lens, br, wr_scale, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    v = valid_mask(lens, L)
    p = {'enc': torch.randn(B, L, D, generator=g) * v[:, :, None], 'dur': torch.randint(0, 7, (B, L), generator=g).float() * v * (256 / 22050),
         'energy': torch.randn(B, L, generator=g) * v, 'pitch': torch.randn(B, L, generator=g) * v, 'lens': list(lens)}
    for n in ('d', 'e', 'p'):
        p['w' + n] = 0.5 * torch.randn(D, 1, 3, generator=g)
        p['b' + n] = 0.1 * torch.randn(D, generator=g)
    p['wr'] = wr_scale * torch.randn(D, generator=g)
    p['br'] = torch.tensor([float(br)])
    return p


# name -> (B, L, br, wr_scale): 16 385 rows (past 4096 blocks of 4, not a multiple of 4); every z > 20, every softplus < 1e-3, both straddled
PREP_CASES = {'large_z': (5, 3277, 40.0, 0.02), 'tiny_softplus': (5, 3277, -14.0, 0.02), 'straddle': (5, 3277, 3.0, 1.0),
              'small': (3, 7, 0.3, 0.1)}


def prep_case(name):
    B, L, br, sc = PREP_CASES[name]
    lens = [L, L - 1, max(L // 2, 1), 1, max(L - 4, 1)][:B]
    return prep_inputs(B, L, lens, br, sc, seed=len(name))


def prep_xs(p, dtype=torch.float64):
    return (cpu(p['enc'], dtype) + conv3(p['energy'], p['we'], p['be'], dtype)) + conv3(p['pitch'], p['wp'], p['bp'], dtype)


def prep_xs_bound(p):
    mag = cpu(p['enc'], torch.float64).abs() + conv3_mag(p['energy'], p['we'], p['be']) + conv3_mag(p['pitch'], p['wp'], p['bp'])
    return (8 + 2) * U * mag


def prep_z(p, xs, dtype=torch.float64):
    """z from the stored xs buffer"""
    return ((cpu(xs, dtype) + conv3(p['dur'], p['wd'], p['bd'], dtype)) * cpu(p['wr'], dtype)).sum(-1) + cpu(p['br'], dtype)


def prep_z_bound(p, xs):
    wr = cpu(p['wr'], torch.float64).abs()
    mag = ((cpu(xs, torch.float64).abs() + conv3_mag(p['dur'], p['wd'], p['bd'])) * wr).sum(-1) + cpu(p['br'], torch.float64).abs()
    return (13 + 2) * U * mag


def softplus(z):
    return torch.where(z > SOFTPLUS_T, z, torch.log1p(torch.exp(z.clamp(max=SOFTPLUS_T))))


def prep_sigma(z, lens, dtype=torch.float64):
    """sigma from the stored z buffer: max(l < len ? softplus(z) : 1, 1e-3f)"""
    z = cpu(z, dtype)
    v = valid_mask(lens, z.shape[1])
    return torch.where(v, softplus(z), torch.ones_like(z)).clamp_min(SIGMA_MIN)


def prep_sigma_bound(sigma64):
    return 8 * U * sigma64


# ---------------------------------------------------------------------------------------------------------------------------------------
# forward: weights and x_up
# ---------------------------------------------------------------------------------------------------------------------------------------
def fit_total(d, n, target, hi):
    """adjust the last durations of d[:n] (each kept in [0, hi]) until they sum to ``target``"""
    d = d.clone()
    k = n - 1
    while int(d[:n].sum()) != target:
        s = int(d[:n].sum())
        if s > target and d[k] > 0:
            d[k] -= 1
        elif s < target and d[k] < hi:
            d[k] += 1
        else:
            k = k - 1 if k > 0 else n - 1
    return d


def _up_common(g, B, L, lens, dur, T, sigma=None):
    v = valid_mask(lens, L)
    dur = dur * v
    mu, totals = scan_ref(dur)
    if sigma is None:
        sigma = torch.where(v, 0.5 + 3.5 * torch.rand(B, L, generator=g), torch.ones(B, L))
    xs = torch.randn(B, L, D, generator=g) * v[:, :, None]
    T = int(totals.max()) if T is None else T
    dxup = torch.randn(B, max(T, 1), D, generator=g)
    return {'B': B, 'L': L, 'T': max(T, 1), 'lens': list(lens), 'dur_int': dur, 'mu': mu, 'totals': totals, 'sigma': sigma.float(), 'xs': xs,
            'dxup': dxup, 'base_dxs': torch.zeros(B, L, D), 'base_dsigma': torch.zeros(B, L)}


def upsample_case(name):
    """The rounded tier's inputs.  sigma in [0.5, 4] and durations <= 6 keep every frame below an utterance's total comparable."""
    g = torch.Generator().manual_seed(300 + sum(map(ord, name)))
    if name == 'a':                        # a one-symbol row of duration 0 (total 0), T no multiple of 16, gradient nonzero on every frame
        B, L, lens = 4, 14, [14, 13, 6, 1]
        dur = torch.randint(0, 7, (B, L), generator=g)
        dur[3] = 0
        dur[0] = fit_total(dur[0], 14, 43, 6)
        dur[1] = fit_total(dur[1], 13, min(int(dur[1, :13].sum()), 40), 6)
        dur[2] = fit_total(dur[2], 6, min(int(dur[2, :6].sum()), 40), 6)
        c = _up_common(g, B, L, lens, dur, None)
        assert c['T'] == 43 and int(c['totals'][3]) == 0
    elif name == 'b':                      # total 1 mod 32; a row ending on a tile edge, two tiles below T; accumulate onto a base
        B, L, lens = 2, 70, [70, 33]
        dur = torch.randint(0, 7, (B, L), generator=g)
        dur[0] = fit_total(dur[0], 70, 225, 6)
        dur[1] = fit_total(dur[1], 33, 96, 6)
        c = _up_common(g, B, L, lens, dur, None)
        assert c['T'] == 225 and c['T'] % 32 == 1 and int(c['totals'][1]) % 32 == 0 and c['T'] - int(c['totals'][1]) >= 64
        c['dxup'][1, 96:] = 0
        c['base_dxs'] = dyadic(g, (B, L, D), 64, 16)
        c['base_dsigma'] = dyadic(g, (B, L), 64, 16)
    elif name in ('c416', 'c417'):         # the two tile widths of the backward
        L = int(name[1:])
        c = _up_common(g, 1, L, [L], torch.randint(0, 3, (1, L), generator=g), None)
    elif name == 'd':                      # the bucketed form: allocated L = 32 and T = 128 above every length and total
        B, L, lens = 3, 32, [20, 11, 1]
        dur = torch.randint(0, 5, (B, L), generator=g)
        dur[2, 0] = 3
        c = _up_common(g, B, L, lens, dur, 128)
        assert int(c['totals'].max()) <= 90
        c['dxup'] = c['dxup'] * (torch.arange(128)[None, :, None] < c['totals'][:, None, None])
        c['base_dxs'] = dyadic(g, (B, L, D), 64, 16)
        c['base_dsigma'] = dyadic(g, (B, L), 64, 16)
    else:
        raise KeyError(name)
    return c


ROUNDED_CASES = ('a', 'b', 'c416', 'c417', 'd')


def onehot_case():
    """sigma = 1e-3, durations in {0, 1, 3}, dyadic xs and gradient: every weight is exactly 1 at the centre frame of an odd-duration
    symbol and exactly 0 elsewhere, so every output is exact in any summation order"""
    g = torch.Generator().manual_seed(77)
    B, L, lens = 3, 100, [100, 77, 1]
    dur = torch.tensor([0, 1, 3])[torch.randint(0, 3, (B, L), generator=g)]
    dur[2, 0] = 1
    c = _up_common(g, B, L, lens, dur, None, sigma=torch.full((B, L), 1e-3))
    v = valid_mask(lens, L)
    c['xs'] = dyadic(g, (B, L, D), 16, 8) * v[:, :, None]
    c['dxup'] = dyadic(g, (B, c['T'], D), 8, 4)
    return c


def onehot_expected(c):
    """(weights, x_up, dxs) exactly, from the integer durations alone"""
    B, L, T = c['B'], c['L'], c['T']
    w = torch.zeros(B, L, T)
    start = torch.cumsum(c['dur_int'], 1) - c['dur_int']
    for b in range(B):
        for l in range(c['lens'][b]):
            d = int(c['dur_int'][b, l])
            if d % 2 == 1:
                w[b, l, int(start[b, l]) + d // 2] = 1.0
    xup = torch.einsum('blt,bld->btd', w, c['xs'])
    dxs = torch.einsum('blt,btd->bld', w, c['dxup'])
    return w, xup, dxs


def weights_ref(mu, sigma, lens, T, dtype=torch.float64):
    """p, den, w as the kernel and the oracle state them: (B, L, T), (B, T), (B, L, T)"""
    mu, sigma = cpu(mu, dtype), cpu(sigma, dtype)
    v = valid_mask(lens, mu.shape[1])[:, :, None]
    t = torch.arange(T, dtype=dtype) + 0.5
    d = t[None, None, :] - mu[:, :, None]
    s = sigma[:, :, None]
    p = torch.exp(-(d * d) / (2 * (s * s)) - torch.log(s) - LOG_SQRT_2PI)
    p = torch.where(v, p, torch.zeros_like(p))
    den = p.sum(1) + 1e-20
    return p, den, p / den[:, None, :]


def weights_bound(mu, sigma, lens, T):
    """(w64, bound, compared (B, T)); the bound is zero for l >= len: those weights must be exactly zero"""
    mu64, s = cpu(mu, torch.float64), cpu(sigma, torch.float64)[:, :, None]
    L = mu64.shape[1]
    p, den, w = weights_ref(mu, sigma, lens, T)
    t = torch.arange(T, dtype=torch.float64) + 0.5
    d = t[None, None, :] - mu64[:, :, None]
    E = (d * d) / (2 * s * s) + torch.log(s).abs() + 0.92
    rel_p = (8 * E + 4) * U
    rel_den = (p * rel_p).sum(1) / den + (L + 2) * U
    bound = w * (rel_p + rel_den[:, None, :] + 2 * U) + F32_TINY / den[:, None, :]
    bound = torch.where(valid_mask(lens, L)[:, :, None], bound, torch.zeros_like(bound))
    return w, bound, den >= DEN_MIN


def xup_ref(w, xs, dtype=torch.float64):
    return torch.einsum('blt,bld->btd', cpu(w, dtype), cpu(xs, dtype))


def xup_bound(w64, wbound, xs, lens):
    ax = cpu(xs, torch.float64).abs()
    nk = torch.tensor([((min(n, ax.shape[1]) + 3) // 4 + 1) & ~1 for n in lens], dtype=torch.float64)
    return torch.einsum('blt,bld->btd', wbound, ax) + ((2 * nk + 3) * U)[:, None, None] * torch.einsum('blt,bld->btd', w64, ax)


def check_forward(c, w_got, xup_got):
    """-> dict of worst ratios; asserts the frame conditions (every frame below a total compared; the others finite, in [0, 1], column
    sum <= 1 + 1e-5)"""
    w64, wb, compared = weights_bound(c['mu'], c['sigma'], c['lens'], c['T'])
    T = c['T']
    below = torch.arange(T)[None, :] < c['totals'][:, None]
    left_out = int((below & ~compared).sum())
    assert left_out == 0, f'{left_out} frames below their utterance total have a float64 denominator under 2^-60'
    wg = cpu(w_got, torch.float64)
    assert bool(torch.isfinite(wg).all()) and float(wg.min()) >= 0 and float(wg.max()) <= 1, 'weights outside [0, 1]'
    assert float(wg.sum(1).max()) <= 1 + 1e-5, 'a column of weights sums to more than 1 + 1e-5'
    assert bool(torch.isfinite(cpu(xup_got)).all())
    rw, iw = worst_ratio(w_got, w64, wb, compared[:, None, :])
    xb = xup_bound(w64, wb, c['xs'], c['lens'])
    rx, ix = worst_ratio(xup_got, xup_ref(w64, c['xs']), xb, compared[:, :, None])
    return {'weights': rw, 'weights_at': iw, 'xup': rx, 'xup_at': ix, 'compared': int(compared.sum()), 'frames': compared.numel()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# backward: dxs, dsigma
# ---------------------------------------------------------------------------------------------------------------------------------------
def bwd_ref(c, weights, dtype=torch.float64, dxup=None, sigma=None):
    """(dxs, dsigma) gradients (without the base) from the stored weights buffer; rows l >= len are zero"""
    L, T = c['L'], c['T']
    v = valid_mask(c['lens'], L)
    g = cpu(c['dxup'] if dxup is None else dxup, dtype)
    x = cpu(c['xs'], dtype) * v[:, :, None]
    w = cpu(weights, dtype) * v[:, :, None]
    mu, s = cpu(c['mu'], dtype)[:, :, None], cpu(c['sigma'] if sigma is None else sigma, dtype)[:, :, None]
    dw = torch.einsum('blc,btc->blt', x, g)
    inner = (dw * w).sum(1)
    dlp = w * (dw - inner[:, None, :])
    d = (torch.arange(T, dtype=dtype) + 0.5)[None, None, :] - mu
    f = (d * d) * (1 / (s * s * s)) - 1 / s
    dsigma = torch.where(v, (dlp * f).sum(2), torch.zeros(1, dtype=dtype))
    dxs = torch.einsum('blt,btc->blc', w, g)
    return dxs, dsigma


def bwd_bounds(c, weights):
    L, T = c['L'], c['T']
    TT = bwd_tile(L)
    LG, tiles = 256 // TT, -(-T // TT)
    v = valid_mask(c['lens'], L)
    g = cpu(c['dxup'], torch.float64).abs()
    x = cpu(c['xs'], torch.float64).abs() * v[:, :, None]
    w = cpu(weights, torch.float64) * v[:, :, None]
    mu, s = cpu(c['mu'], torch.float64)[:, :, None], cpu(c['sigma'], torch.float64)[:, :, None]
    A = torch.einsum('blc,btc->blt', x, g)
    Ain = (A * w).sum(1)
    d = (torch.arange(T, dtype=torch.float64) + 0.5)[None, None, :] - mu
    S = (w * ((d * d) / (s * s * s) + 1 / s) * (A + Ain[:, None, :])).sum(2)
    n_ds = 65 + -(-L // LG) + LG + TT + tiles + 1
    b_ds = (n_ds + 2 + 8) * U * (S + cpu(c['base_dsigma'], torch.float64).abs())
    b_ds = torch.where(v, b_ds, torch.zeros_like(b_ds))                       # rows l >= len keep their bits
    n_dx = TT + tiles + 1
    b_dx = (n_dx + 2) * U * (torch.einsum('blt,btc->blc', w, g) + cpu(c['base_dxs'], torch.float64).abs())
    b_dx = torch.where(v[:, :, None], b_dx, torch.zeros_like(b_dx))
    return b_dx, b_ds


def check_backward(c, weights, dxs_got, dsigma_got):
    dxs, dsigma = bwd_ref(c, weights)
    b_dx, b_ds = bwd_bounds(c, weights)
    rx, ix = worst_ratio(dxs_got, cpu(c['base_dxs'], torch.float64) + dxs, b_dx)
    rs, i_s = worst_ratio(dsigma_got, cpu(c['base_dsigma'], torch.float64) + dsigma, b_ds)
    return {'dxs': rx, 'dxs_at': ix, 'dsigma': rs, 'dsigma_at': i_s}


# ---------------------------------------------------------------------------------------------------------------------------------------
# symbol backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def sym_bwd_inputs(B=13, L=79, seed=0):
    """1027 rows (past 256 blocks of 4, not a multiple of 4).  z is an input: values either side of 20 and of Z_GATE are planted, at 1
    ulp (excluded around the gate), 6 ulp and further (compared)."""
    g = torch.Generator().manual_seed(400 + seed)
    lens = [L - (3 * b) % 17 for b in range(B)]
    lens[-1] = 1
    v = valid_mask(lens, L)
    z = 8 * torch.randn(B, L, generator=g)
    plant = []
    for centre in (SOFTPLUS_T, f32(Z_GATE)):
        for k in (-4096, -64, -6, -1, 0, 1, 6, 64, 4096):
            plant.append(f32(centre) + k * ulp32(centre))
    z.view(-1)[:len(plant)] = torch.tensor(plant, dtype=torch.float32)          # row 0 is full length
    p = {'B': B, 'L': L, 'lens': lens, 'z': z, 'dsigma': torch.randn(B, L, generator=g) * v, 'dxs_in': torch.randn(B, L, D, generator=g) * v[:, :, None],
         'xs': torch.randn(B, L, D, generator=g) * v[:, :, None], 'dur': torch.randint(0, 7, (B, L), generator=g).float() * v * (256 / 22050),
         'wd': 0.5 * torch.randn(D, 1, 3, generator=g), 'bd': 0.1 * torch.randn(D, generator=g), 'wr': 0.1 * torch.randn(D, generator=g)}
    return p


def sym_dz(p, dtype=torch.float64):
    """(dz, compared): dz = dsigma * sigmoid(z) (1 beyond 20) where l < len and softplus(z) >= 1e-3f; entries whose z is within 4 ulp of
    the gate Z_GATE are left out of the comparison (at 20 both sides branch on the same fp32 z: nothing is ambiguous there)"""
    z, ds = cpu(p['z'], dtype), cpu(p['dsigma'], dtype)
    v = valid_mask(p['lens'], p['L'])
    gate = v & (softplus(z) >= SIGMA_MIN)
    sig = torch.where(z > SOFTPLUS_T, torch.ones_like(z), 1 / (1 + torch.exp(-z)))
    dz = torch.where(gate, ds * sig, torch.zeros_like(z))
    near = (cpu(p['z'], torch.float64) - Z_GATE).abs() <= 4 * ulp32(Z_GATE)
    return dz, ~(near & v)


def sym_rest(p, dz, dtype=torch.float64):
    """(dxs_out, dwr, dbr) from the stored dz buffer"""
    dz = cpu(dz, dtype)
    t = cpu(p['xs'], dtype) + conv3(p['dur'], p['wd'], p['bd'], dtype)
    return cpu(p['dxs_in'], dtype) + dz[:, :, None] * cpu(p['wr'], dtype), (dz[:, :, None] * t).sum((0, 1)), dz.sum().reshape(1)


def sym_bounds(p, dz):
    rows = p['B'] * p['L']
    grid = min((rows + 3) // 4, SYM_BWD_BLOCKS)
    n = 4 + -(-rows // (4 * grid)) + 2 + grid
    dz = cpu(dz, torch.float64).abs()
    mag = cpu(p['xs'], torch.float64).abs() + conv3_mag(p['dur'], p['wd'], p['bd'])
    b_out = 3 * U * (cpu(p['dxs_in'], torch.float64).abs() + dz[:, :, None] * cpu(p['wr'], torch.float64).abs())
    return b_out, (n + 2) * U * (dz[:, :, None] * mag).sum((0, 1)), (n + 2) * U * dz.sum().reshape(1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------------------------------
# name -> (B, M, T, lens, rows_exist, e_per_total)
LOSS_CASES = {
    'one_frame': (3, 80, 1, [1, 1, 1], None, 0),
    'edge64': (3, 80, 65, [65, 64, 1], None, 0),
    'edge256': (3, 80, 257, [257, 256, 100], None, 0),
    'rows_exist': (3, 80, 192, [130, 64, 5], [130, 70, 64], 0),
    'five_bins': (2, 5, 65, [65, 30], None, 0),
    'batch300': (300, 80, 3, [1 + (7 * b) % 3 for b in range(300)], None, 1),
}


def loss_case(name):
    """Mels as the model hands them over: target in [-11.5, 2], prediction = target + noise, both ZERO at and beyond the length (the
    decoder masks its output and the data pipeline pads with zeros: the kernels sum over every stored frame and rely on it).  About
    1 % of the cells below the length have prediction == target (sign 0)."""
    B, M, T, lens, rows_exist, ept = LOSS_CASES[name]
    g = torch.Generator().manual_seed(500 + sum(map(ord, name)))
    v = valid_mask(lens, T)[:, None, :]
    mt = (-5 + 2 * torch.randn(B, M, T, generator=g)).clamp(-11.5, 2) * v
    same = torch.rand(B, M, T, generator=g) < 0.01
    mp = torch.where(same, mt, mt + 0.3 * torch.randn(B, M, T, generator=g)) * v
    return {'B': B, 'M': M, 'T': T, 'lens': list(lens), 'rows_exist': rows_exist, 'e_per_total': ept, 'mp': mp, 'mt': mt,
            'c_l1': f32(1.0 / (M * B)), 'c_l2': f32(1.0 / (M * B)), 'c_e': f32(0.05) if ept else f32(0.05 / sum(lens))}


def mel_stats_ref(mp, mt, dtype=torch.float64):
    p, q = cpu(mp, dtype), cpu(mt, dtype)
    d = p - q
    return {'l1': d.abs().sum((1, 2)), 'l2': (d * d).sum((1, 2)), 'ep': torch.sqrt((torch.exp(p) ** 2).sum(1)), 'et': torch.sqrt((torch.exp(q) ** 2).sum(1))}


def mel_stats_bounds(ref, M, T):
    n = -(-M // 4) + 6 + 2 + -(-T // MEL_TT)
    ne = -(-M // 4) + 2 + 8
    return {'l1': (n + 2) * U * ref['l1'], 'l2': (n + 4) * U * ref['l2'], 'ep': ne * U * ref['ep'], 'et': ne * U * ref['et']}


def pool5(x):
    """sum over the window [t - 2, t + 2], zero outside the stored frames"""
    p = F.pad(x, (2, 2))
    T = x.shape[-1]
    return sum(p[..., k:k + T] for k in range(5))


def energy_ref(ep, et, lens, rows_exist, dtype=torch.float64, ignore_rows_exist=False, drop=None):
    """(des, esum, diff) from the stored ep / et buffers.  Planted errors: ``ignore_rows_exist``; ``drop`` = (b, t, u): frame u is
    missing from the window of frame t."""
    ep, et = cpu(ep, dtype), cpu(et, dtype)
    B, T = ep.shape
    if rows_exist is not None and not ignore_rows_exist:
        ex = valid_mask([min(r, T) for r in rows_exist], T)
        ep, et = torch.where(ex, ep, torch.zeros_like(ep)), torch.where(ex, et, torch.zeros_like(et))
    a, c = pool5(ep), pool5(et)
    if drop is not None:
        b, t, u = drop
        a, c = a.clone(), c.clone()
        a[b, t] -= ep[b, u]
        c[b, t] -= et[b, u]
    diff = a / 5 - c / 5
    v = valid_mask(lens, T)
    zero = torch.zeros_like(diff)
    return torch.where(v, 2 * diff, zero), torch.where(v, diff * diff, zero).sum().reshape(1), diff


def energy_bounds(ep, et, lens, rows_exist):
    ep, et = cpu(ep, torch.float64), cpu(et, torch.float64)
    B, T = ep.shape
    if rows_exist is not None:
        ex = valid_mask([min(r, T) for r in rows_exist], T)
        ep, et = torch.where(ex, ep, torch.zeros_like(ep)), torch.where(ex, et, torch.zeros_like(et))
    eps = 9 * U * (pool5(ep.abs()) + pool5(et.abs())) / 5
    _, esum, diff = energy_ref(ep, et, lens, None)
    v = valid_mask(lens, T)
    zero = torch.zeros_like(eps)
    n = 6 + 2 + B * -(-T // 256)
    return torch.where(v, 2 * eps, zero), torch.where(v, 2 * diff.abs() * eps + eps * eps, zero).sum().reshape(1) + (n + 2) * U * esum


def mel_grad_ref(c, ep, des, dtype=torch.float64, c_scale=1.0, drop=None):
    """dmel from the stored ep / des buffers.  ``c_scale``: multiplies the three coefficients as the C entry receives them."""
    p, q = cpu(c['mp'], dtype), cpu(c['mt'], dtype)
    ep, des = cpu(ep, dtype), cpu(des, dtype)
    lens = torch.tensor(c['lens'], dtype=dtype)
    c1, c2, ce = (f32(c[k] * c_scale) for k in ('c_l1', 'c_l2', 'c_e'))
    if c['e_per_total']:
        ce = ce / float(sum(c['lens']))
    a = pool5(des)
    if drop is not None:
        b, t, u = drop
        a = a.clone()
        a[b, t] -= des[b, u]
    d = p - q
    inv = (1 / lens)[:, None, None]
    t1, t2 = c1 * torch.sign(d) * inv, c2 * 2 * d * inv
    t3 = (ce * (a / 5) / ep)[:, None, :] * torch.exp(p) ** 2
    bound = 8 * U * (t1.abs() + t2.abs()) + 14 * U * (abs(ce) * (pool5(des.abs()) / 5) / ep)[:, None, :] * torch.exp(p) ** 2
    return t1 + t2 + t3, bound


def pitch_inputs(B, T, lens, seed=0, all_unvoiced=False):
    g = torch.Generator().manual_seed(600 + seed)
    gt = (4.5 + 0.5 * torch.randn(B, T, generator=g)) * (torch.rand(B, T, generator=g) > 0.3)
    gt[:, T - 1] = 4.25                      # the last stored frame is voiced: in 'edge256' it is the only frame of the second block
    if all_unvoiced:
        gt = torch.zeros(B, T)
    return {'B': B, 'T': T, 'lens': list(lens), 'pp': 4.5 + 0.7 * torch.randn(B, T, generator=g), 'gt': gt}


PITCH_CASES = {'one_frame': (3, 1, [1, 1, 1]), 'edge256': (3, 257, [257, 256, 100])}


def pitch_ref(c, dtype=torch.float64):
    """(sum of squares, count, bound of the sum)"""
    pp, gt = cpu(c['pp'], dtype), cpu(c['gt'], dtype)
    m = valid_mask(c['lens'], c['T']) & (gt != 0)
    e = torch.where(m, (pp - gt) ** 2, torch.zeros_like(pp))
    n = 6 + 2 + c['B'] * -(-c['T'] // 256)
    return e.sum(), float(m.sum()), (n + 4) * U * float(e.double().sum())


def pitch_grad_ref(c, count, scale, dtype=torch.float64):
    """dpp from the stored count: scale * 2 (pp - gt) mask / (count + 1e-5f); (value, bound)"""
    pp, gt = cpu(c['pp'], dtype), cpu(c['gt'], dtype)
    m = valid_mask(c['lens'], c['T']) & (gt != 0)
    v = torch.where(m, f32(scale) * 2 * (pp - gt) / (float(count) + EPS_COUNT), torch.zeros_like(pp))
    return v, 6 * U * v.abs().double()


def finalize_inputs(B, lens, seed=0, S=3, n_pm=16):
    g = torch.Generator().manual_seed(700 + seed)
    lf = torch.tensor(lens, dtype=torch.float32)
    return {'B': B, 'M': 80, 'lens': list(lens), 'ce': torch.tensor([1.1]), 'spk_w': 0.37, 'dlogits': 0.2 * torch.randn(B, S, generator=g),
            'pm': 0.5 * torch.randn(n_pm, generator=g), 'pmw': 0.013, 'l1sum': 80 * lf * (0.3 + torch.rand(B, generator=g)),
            'l2sum': 80 * lf * (0.1 + torch.rand(B, generator=g)), 'msw': 1.5, 'esum': torch.tensor([3.7 * float(lf.sum())]), 'ecw': 0.05,
            'psum': torch.tensor([0.8 * 41.0, 41.0]), 'pcw': 0.15, 'grad_scale': 0.25}


FINALIZE_SWITCHES = (None, 'ce', 'pm', 'esum', 'psum')


def finalize_ref(f, off=None, dtype=torch.float64, gs_scale=1.0):
    """-> dict of (value, bound): terms (7), total, d_spk, d_pm.  ``off``: the argument handed in as NULL (with ce the logits go too, with
    pm its gradient).  ``gs_scale``: multiplies grad_scale as the C entry receives it."""
    B, M = f['B'], f['M']
    get = lambda k: None if k == off else cpu(f[k], dtype)
    ce, pm, esum, psum = get('ce'), get('pm'), get('esum'), get('psum')
    lens = torch.tensor(f['lens'], dtype=dtype)
    w, pmw, msw, ecw, pcw = (f32(f[k]) for k in ('spk_w', 'pmw', 'msw', 'ecw', 'pcw'))
    gs = f32(f['grad_scale'] * gs_scale)
    nB = -(-B // 256) + 8
    a1, a2 = cpu(f['l1sum'], dtype) / (M * lens), cpu(f['l2sum'], dtype) / (M * lens)
    n = lens.sum()
    cev = ce[0] if ce is not None else torch.zeros((), dtype=dtype)
    t0, t1 = w * cev, cev
    npm = 0 if pm is None else pm.numel()
    nrm = torch.sqrt((pm * pm).sum()) if npm else torch.zeros((), dtype=dtype)
    t2 = pmw * nrm
    t3, t4 = msw * a1.sum() / B, msw * a2.sum() / B
    t5 = esum[0] / n if esum is not None else torch.zeros((), dtype=dtype)
    t6 = psum[0] / (psum[1] + EPS_COUNT) if psum is not None else torch.zeros((), dtype=dtype)
    terms = torch.stack([t0, t1, t2, t3, t4, t5, t6])
    b = [U * abs(float(t0)), 0.0, (-(-max(npm, 1) // 256) + 8 + 6) * U * abs(float(t2)), (nB + 6) * U * abs(msw) * float(a1.abs().sum()) / B,
         (nB + 6) * U * abs(msw) * float(a2.abs().sum()) / B, 3 * U * abs(float(t5)), 3 * U * abs(float(t6))]
    total = t0 + t2 + t3 + t4 + ecw * t5 + pcw * t6
    mags = [abs(float(t0)), abs(float(t2)), abs(float(t3)), abs(float(t4)), abs(ecw * float(t5)), abs(pcw * float(t6))]
    b_total = b[0] + b[2] + b[3] + b[4] + abs(ecw) * b[5] + abs(pcw) * b[6] + (5 + 2 + 2) * U * sum(mags)
    out = {'terms': (terms, torch.tensor(b, dtype=torch.float64)), 'total': (total.reshape(1), torch.tensor([b_total], dtype=torch.float64))}
    if ce is not None:
        v = cpu(f['dlogits'], dtype) * (w * gs)
        out['d_spk'] = (v, 3 * U * v.abs().double())
    if npm:
        v = gs * pmw * pm / nrm
        out['d_pm'] = (v, (-(-npm // 256) + 8 + 8) * U * v.abs().double())
    return out


def cross_entropy_inputs(B, S=3, seed=0):
    g = torch.Generator().manual_seed(800 + seed + B)
    return 3 * torch.randn(B, S, generator=g), torch.randint(0, S, (B,), generator=g)


def cross_entropy_ref(logits, target, dtype=torch.float64):
    """(loss, dlogits, bound of the loss, bound of dlogits)"""
    l = cpu(logits, dtype)
    B, S = l.shape
    tgt = cpu(target).long()
    m = l.max(1).values
    zs = torch.exp(l - m[:, None]).sum(1)
    lse = m + torch.log(zs)
    lt = l.gather(1, tgt[:, None])[:, 0]
    loss = (lse - lt).sum() / B
    onehot = F.one_hot(tgt, S).to(dtype)
    p = torch.exp(l - lse[:, None])
    dl = (p - onehot) / B
    eps = (S + 6) * U * (m.abs() + torch.log(zs).abs()).double()
    n = -(-B // 256) + 8
    b_loss = float(((eps + U * (lse - lt).abs().double()).sum() + (n + 2) * U * (lse - lt).abs().double().sum()) / B)
    b_dl = (p.double() * (eps[:, None] + U * (l - lse[:, None]).abs().double() + 3 * U) + 2 * U * (p - onehot).abs().double()) / B
    return loss.reshape(1), dl, b_loss, b_dl
