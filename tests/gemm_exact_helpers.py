"""Float64 references, per-element bounds and the library's launch plans for the GEMM family (csrc/dx_gemm.hip, csrc/dx_ffpair.hip).

The reference of every checked element is float64 arithmetic on exactly the operands the device multiplies: weights rounded as the
pack rounds them (``w.to(h16)``, RNE), f32-stored activations rounded where the kernel converts them, 16-bit-stored activations as
stored, nothing rounded in f32 mode.  Beside ``y64`` comes ``S = sum |x_k| |w_k| + |bias|`` of the same element (the same
convolution on absolute values), in pre-epilogue units.  With ``g`` the factor the element's epilogue applies,

    fp32-stored output:    |y_dev - y64| <= Q S g
    16-bit-stored output:  |y_dev - y64| <= Q S g + u_h |y64| (+ 2^-25 in fp16: half a subnormal step)

Q = 16 * 2^-24.  The f32 MFMA is a k-ordered fmaf chain measured at 0.75-1.5e-7 sum|a b| for K <= 1024 and 3.5e-7 at K = 4096
(K <= 3072 here); Q is ~2.7 x that, the margin covering the other summation orders (K split inside a workgroup, split-K atomics).
A path whose interior elements sit above Q uniformly may be raised up to Q_CAP = 64 * 2^-24 and no further: at the cap one product
dropped from a K = 3072 sum (median signal 1.7e-4 S) is still ~45 x the bar (test_gemm_exact_cpu.py).
"""
import struct

import torch

U24 = 2.0 ** -24
Q0 = 16 * U24
Q_CAP = 64 * U24
H16 = {'bf16': torch.bfloat16, 'fp16': torch.float16}
U_H = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}
MAX_EXCLUDED = 0.25          # share of a case's elements that may sit in the "either computed or zero" rows
TILE = 128


# ---------------------------------------------------------------------------------------------------------------------------
# operands and float64 references
# ---------------------------------------------------------------------------------------------------------------------------
def operand64(t, mode):
    """float64 copy of what the device multiplies: 16-bit-stored tensors as stored, fp32 ones rounded to the mode's type (RNE)."""
    if mode == 'f32':
        assert t.dtype == torch.float32
        return t.double()
    if t.dtype in (torch.bfloat16, torch.float16):
        assert t.dtype == H16[mode]
        return t.double()
    return t.to(H16[mode]).double()


def effective_weight(w, transpose=False):
    """(Cout, Cin[, taps]) parameter -> the (Cout_eff, Cin_eff, taps) weight of the launch: ``transpose`` (the input-gradient
    convolution, which reads the ``bwd`` image) swaps the channel axes and flips the taps."""
    w3 = w if w.dim() == 3 else w[:, :, None]
    return w3.transpose(0, 1).flip(2).contiguous() if transpose else w3


def _shift(x, s):
    """rows n of the result hold x[n + s], zero outside the batch row"""
    if s == 0:
        return x
    out = torch.zeros_like(x)
    if abs(s) < x.shape[1]:
        if s > 0:
            out[:, :-s] = x[:, s:]
        else:
            out[:, -s:] = x[:, :s]
    return out


def _row_mask(N, limit, device):
    """(B, N, 1) bool: n < limit[b]"""
    return (torch.arange(N, device=device)[None, :] < limit.to(device)[:, None].long())[:, :, None]


def conv64(x64, w64, bias=None, rows_exist=None):
    """(y64, S) of the 'same' convolution, before any epilogue.  x64 (B, N, Cin), w64 (Cout, Cin, taps) float64.
    ``rows_exist`` [B]: input rows at or beyond it read as zero (the output rows there are the caller's business)."""
    assert x64.dtype == torch.float64 and w64.dtype == torch.float64
    B, N, _ = x64.shape
    taps = w64.shape[2]
    pad = (taps - 1) // 2
    if rows_exist is not None:
        x64 = x64 * _row_mask(N, rows_exist, x64.device)
    xa, wa = x64.abs(), w64.abs()
    y = S = None
    for t in range(taps):
        yt = _shift(x64, t - pad) @ w64[:, :, t].T
        st = _shift(xa, t - pad) @ wa[:, :, t].T
        y, S = (yt, st) if y is None else (y + yt, S + st)
    if bias is not None:
        y = y + bias.double()
        S = S + bias.double().abs()
    return y, S


def epilogue64(y, S, *, relu=False, post_scale=None, post_shift=None, aux=None, out_scale=1.0):
    """The epilogue of dx_conv_gemm in float64 -> (y64, g): y = out_scale * [aux > 0] * (post_scale * relu?(y) + post_shift); g is the
    per-channel factor the bound carries through it (the ReLU is 1-Lipschitz, the shift is added exactly)."""
    if relu:
        y = y.clamp_min(0)
    g = torch.full((y.shape[-1],), abs(float(out_scale)), dtype=torch.float64, device=y.device)
    if post_scale is not None:
        y = y * post_scale.double() + post_shift.double()
        g = g * post_scale.double().abs()
    y = y * float(out_scale)
    if aux is not None:
        y = torch.where(aux.double() > 0, y, torch.zeros_like(y))
    return y, g


def wgrad64(dy64, x64, taps, rows_exist=None):
    """(G64, SG, db64, Sb): G[co, ci, tap] = sum_{b, n} dY[b, n, co] X[b, n + tap - pad, ci] and the bias gradient, with their
    magnitude sums over the token axis.  Rows at or beyond ``rows_exist`` read as zero in both operands."""
    B, N, Cout = dy64.shape
    Cin = x64.shape[2]
    pad = (taps - 1) // 2
    if rows_exist is not None:
        m = _row_mask(N, rows_exist, x64.device)
        dy64, x64 = dy64 * m, x64 * m
    dya, xa = dy64.abs(), x64.abs()
    G = torch.empty(Cout, Cin, taps, dtype=torch.float64, device=x64.device)
    SG = torch.empty_like(G)
    for t in range(taps):
        G[:, :, t] = dy64.reshape(B * N, Cout).T @ _shift(x64, t - pad).reshape(B * N, Cin)
        SG[:, :, t] = dya.reshape(B * N, Cout).T @ _shift(xa, t - pad).reshape(B * N, Cin)
    return G, SG, dy64.sum((0, 1)), dya.sum((0, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# the statistic
# ---------------------------------------------------------------------------------------------------------------------------
class Verdict:
    """Outcome of ``check``: ``fail`` marks every element that violates its condition; ``ratio`` is max |err| / (S g) over the
    element-wise region in units of 2^-24 (the 16-bit output rounding allowance taken off first)."""

    def __init__(self, fail, ratio, what):
        self.fail, self.ratio, self.what = fail, ratio, what

    @property
    def ok(self):
        return not bool(self.fail.any())

    def describe(self, limit=12):
        idx = self.fail.nonzero()
        rows = ', '.join(str(tuple(int(v) for v in r)) for r in idx[:limit])
        return f'{self.what}: {idx.shape[0]} of {self.fail.numel()} elements out of bounds (max ratio {self.ratio:.1f} x 2^-24); first at {rows}'

    def assert_ok(self):
        assert self.ok, self.describe()
        return self.ratio


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def check(dev, y64, S, g=1.0, *, q=Q0, out16=None, must=None, exact=None, exact_value=None, between=None, what=''):
    """Per-element verdict of a device result ``dev`` (any float type) against ``y64`` with magnitude sums ``S``.

    must     rows checked element-wise (default: every row no other region claims)
    exact    rows that must hold ``exact_value`` (a tensor of dev's type: compared bitwise) or, without one, exactly zero
    between  rows that may hold either: the exact value, or an in-bound result (rows between len + halo and the kernel's tile edge)
    The regions are (B, N, 1)-broadcastable bool tensors and must cover every element once.  No more than MAX_EXCLUDED of the
    elements may sit in ``between``."""
    assert q <= Q_CAP * (1 + 1e-12), 'the bar of a path may be raised to the cap and no further'
    shape = dev.shape
    full = lambda m: torch.zeros(shape, dtype=torch.bool, device=dev.device) if m is None else m.expand(shape)
    exact_m, between_m = full(exact), full(between)
    must_m = ~(exact_m | between_m) if must is None else must.expand(shape)
    assert bool((must_m.int() + exact_m.int() + between_m.int() == 1).all()), 'regions must cover every element exactly once'
    share = float(between_m.float().mean())
    assert share < MAX_EXCLUDED, f'{what}: {share:.1%} of the elements are excluded from the element-wise check (cap {MAX_EXCLUDED:.0%})'
    d64 = dev.double()
    err = (d64 - y64).abs()
    allow = torch.zeros_like(err)
    if out16 is not None:
        assert dev.dtype == H16[out16]
        allow = U_H[out16] * y64.abs() + (2.0 ** -25 if out16 == 'fp16' else 0.0)
    scale = S * g
    inb = (err <= q * scale + allow) & torch.isfinite(d64)
    if exact_value is None:
        same = (d64 == 0)
    else:
        assert exact_value.dtype == dev.dtype
        same = _bits(dev) == _bits(exact_value)
    fail = (must_m & ~inb) | (exact_m & ~same) | (between_m & ~(same | inb))
    r = ((err - allow).clamp_min(0) / scale.clamp_min(1e-300))[must_m & (scale > 0)]
    ratio = float(r.max()) / U24 if r.numel() else 0.0
    return Verdict(fail, ratio, what)


def row_regions(N, lens, halo, device, tile=TILE):
    """(must, beyond, between) of a launch that skips token tiles at or beyond len + halo: rows below len + halo are computed, whole
    128-token tiles beyond them are exactly zero / untouched, the rows in between may be either (the tile is the kernel's business)."""
    lim = (lens.to(device).long() + halo).clamp(max=N)
    n = torch.arange(N, device=device)[None, :, None]
    must = n < lim[:, None, None]
    beyond = n >= ((lim + tile - 1) // tile * tile)[:, None, None]
    return must, beyond, ~must & ~beyond


def pick_lens(B, N, tile, rotate=0, open_halo=None):
    """Lengths for B batch rows out of {N, tile + 1, tile - 1, 1, tile} (clipped to 1..N, deduplicated), starting ``rotate`` entries in.
    ``open_halo`` (launches that leave the rows between len + halo and the tile edge open): while those rows are 20 % of the case
    or more, the length that opens the most rows is replaced by the full length, so the exclusion cap holds by construction."""
    cand = []
    for v in (N, tile + 1, tile - 1, 1, tile):
        v = max(1, min(N, v))
        if v not in cand:
            cand.append(v)
    lens = [cand[(rotate + i) % len(cand)] for i in range(B)]
    if open_halo is not None:
        def opened(n):
            lim = min(n + open_halo, N)
            return min(_roundup(lim, tile), N) - lim
        while sum(opened(n) for n in lens) >= 0.2 * B * N:
            lens[max(range(B), key=lambda i: opened(lens[i]))] = N
    return lens


# ---------------------------------------------------------------------------------------------------------------------------
# the host-side launch plan: the library's own answer (the dx_*_plan entry points, include/daft_exprt_hip.h), restated nowhere
# ---------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _roundup(a, b):
    return _cdiv(a, b) * b


OPERAND_MODE = {'f32': 0, 'bf16': 1, 'fp16': 1, 'bf16x3': 2}
# how the tables of test_gemm_exact_gpu.py name a plan's kernel (Plan.kernel: the header's DX_K_* names)
PATH = {'conv_gemm_f32': 'f32_{tok}', 'conv_gemm_h16': 'h16_{tok}', 'conv_gemm_split': 'split_{tok}', 'conv_ws': 'ws', 'conv_dk': 'dk',
        'wgrad_f32': 'f32', 'wgrad_split': 'split', 'wgrad_h16': 'narrow', 'wgrad_h16_wide': 'wide'}


def _plan(entry, mode, *args):
    from ubisoft_laforge_daft_exprt_amd import _lib
    return _lib.plan(entry + ('_f16' if mode == 'fp16' else ''), *args)


def path(plan):
    return PATH[plan.kernel].format(tok=plan.tok)


def conv_plan(mode, B, N, Cin, Cout, taps, ldx=None):
    """what dx_conv_gemm launches for this shape (``.coutp`` / ``.cinp``: the pack's padded dimensions)"""
    return _plan('dx_conv_gemm_plan', mode, B, N, Cin, Cout, taps, OPERAND_MODE[mode], Cin if ldx is None else ldx)


def wgrad_plan(mode, B, N, Cin, Cout, taps, dy16=False, x16=False, ldx=None, ldy=None):
    """what dx_conv_wgrad launches (``.chunk``: tokens per K chunk)"""
    return _plan('dx_conv_wgrad_plan', mode, B, N, Cin, Cout, taps, OPERAND_MODE[mode], Cin if ldx is None else ldx, Cout if ldy is None else ldy,
                 int(dy16), int(x16))


def wgrad_batched_plan(mode, taps, jobs, dy16=False, x16=False):
    """what dx_conv_wgrad_batched launches for jobs of these (B, N, Cin, Cout) (``.rounds``: rounds of workgroups)"""
    import ctypes
    recs = b''.join(struct.pack('<5Q8iQ', 0, 0, 0, 0, 0, Cout, Cin, B, N, Cin, Cout, -1, 0, 0) for B, N, Cin, Cout in jobs)     # DxWgradJob, pointers null
    buf = ctypes.create_string_buffer(recs)
    return _plan('dx_conv_wgrad_batched_plan', mode, ctypes.addressof(buf), len(jobs), taps, int(dy16), int(x16))


def ff_pair_plan(B, N, mode='bf16'):
    """what the fused feed-forward pair launches (``.tok``: output tokens per workgroup)"""
    return _plan('dx_ff_pair_plan', mode, B, N)


LIVE_TILE_ROWS = 1024        # DK_MAX_B: batch rows the weight-stationary / deep-K kernels number live token tiles for


def plain_tile_order(B):
    """True when the weight-stationary / deep-K kernels fall back to the plain (b, tile) order and per-row limits read from memory.
    Decided inside the kernels (``a.B <= DK_MAX_B`` in conv_ws_kernel / conv_dk_kernel), not by host code: no plan reports it."""
    return B > LIVE_TILE_ROWS


PACK_MAX = 60                # descriptors per launch of dx_pack_weights_host


def pack_descriptor(w_ptr, fwd_ptr, bwd_ptr, cout, cin, taps, dims):
    """one 56-byte record of dx_pack_weights_batched / dx_pack_weights_host:
    {const float* W; void* fwd; void* bwd; int32 Cout, Cin, taps, CoutP_f, CinP_f, CinP_b, CoutP_b, pad}"""
    return struct.pack('<QQQ8i', w_ptr, fwd_ptr, bwd_ptr, cout, cin, taps, dims[0], dims[1], dims[2], dims[3], 0)
