"""Attention dropout beyond one tile.  No mask is stored: the forward, the dQ kernel and the dK/dV kernel each rebuild their keep / drop
decisions from (seed, utterance * head, query row, key), in three kernel families (exact f32, split bf16, the templated 16-bit kernels).
Here the mask is READ OUT of the forward at any N (``helpers.recover_keep``), compared with the documented counter rebuilt on the host
(``helpers.host_attention_keep``), and the forward and each of dQ, dK, dV are compared with float64 under that mask: several query and
key tiles, ragged last tiles, more than two utterances, 1 / 2 / 4 heads, strided rows, a seed offset.  A backward whose mask disagrees
with the forward's in any tile gives O(1) errors in that tile's rows.

The CPU tests prove the read-out protocol, its decode thresholds and the reference-only emulation without a GPU."""
import math

import pytest
import torch

from tests import helpers

DEV = 'cuda'
SEED = 0xABCDEF1234
H16 = {'bf16': torch.bfloat16, 'fp16': torch.float16}

# forward / backward bars per mode: test_kernels_gpu.test_attention_forward_backward and test_bf16x3_gpu.test_attention_bf16x3_vs_float64,
# here applied to ctx, lse, dQ, dK and dV one by one (max |error| over the component / max |reference| over the component), and to each
# gradient once more per utterance of at least 64 tokens
BARS = {'f32': (3e-6, 1e-5), 'bf16x3': (5e-5, 5e-5), 'bf16': (2e-2, 3e-2), 'fp16': (3e-3, 5e-3)}
# decode threshold of the read-out: the 16-bit modes round the probability and a 16-bit context once each (< 2 * 2^-9 relative in bf16)
DECODE_TOL = {'f32': 1e-4, 'bf16x3': 1e-4, 'bf16': 0.05, 'fp16': 0.05}

SHAPES = {
    'A': dict(N=64, lens=[64, 48]),                                     # the single-tile anchor
    'B': dict(N=150, lens=[150, 149, 7]),
    'C': dict(N=300, lens=[300, 257, 129, 64, 1]),                      # 5 x 5 tiles; lengths on, just past and inside tile edges; one token
    'D': dict(N=1000, lens=[1000, 881, 513]),                           # the C2 decoder's scale: 16 key tiles
    'E': dict(N=130, lens=[130, 129, 128, 65, 64, 63, 2, 1, 100], ordered=True),   # 9 utterances (numbering pads to 8), longest first
    'C_p50': dict(N=300, lens=[300, 257, 129, 64, 1], p=0.5),
    'B_h1': dict(N=150, lens=[150, 149, 7], heads=1),
    'B_h4': dict(N=150, lens=[150, 149, 7], heads=4),
    'B_strided': dict(N=150, lens=[150, 149, 7], strided=True),         # qkv rows inside a wider tensor: ld = 3 D + 8
}


def variants(mode):
    """(name, qkv storage, ctx / dctx storage, dqkv storage): the template instantiations dx_attention_fwd / dx_attention_bwd dispatch to"""
    if mode not in H16:
        return [('f32 storage', torch.float32, torch.float32, torch.float32)]
    h = H16[mode]
    return [('f32 qkv, f32 ctx, f32 dqkv', torch.float32, torch.float32, torch.float32),
            ('16-bit qkv, f32 ctx, 16-bit dqkv', h, torch.float32, h),
            ('all 16-bit', h, h, h)]


def err(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def keep_rate_failures(keep, lens, heads, p):
    """|mean(keep) - (1 - p)| <= 6 sqrt(p (1 - p) / n), over all valid decisions and per (utterance, head) of at least 128 tokens"""
    bad = []
    total = cnt = 0
    for b, n in enumerate(lens):
        for h in range(heads):
            k = keep[b, h, :n, :n]
            total, cnt = total + int(k.sum()), cnt + n * n
            if n >= 128 and abs(k.double().mean().item() - (1 - p)) > 6 * math.sqrt(p * (1 - p) / (n * n)):
                bad.append(('keep rate', b, h, k.double().mean().item()))
    if abs(total / cnt - (1 - p)) > 6 * math.sqrt(p * (1 - p) / cnt):
        bad.append(('keep rate over all', total / cnt, cnt))
    return bad


# ------------------------------------------------------------------------------------------------------------------------------------
# without a GPU: the read-out protocol, the host mask and the emulation
# ------------------------------------------------------------------------------------------------------------------------------------
def planted_forward(keep, lens, heads, p, h16):
    def fwd(qkv):
        ctx = helpers.attention_emulation(qkv, lens, heads, keep=keep, p=p, h16=h16)
        return ctx if h16 is None else ctx.to(h16)          # a 16-bit stored context rounds once more
    return fwd


@pytest.mark.parametrize('rounding', [None, 'bf16', 'fp16'])
@pytest.mark.parametrize('N,lens,heads,p', [(1000, [1000, 881, 513], 2, 0.1), (130, [130, 65, 64, 1], 4, 0.5), (64, [64, 48], 1, 0.25)])
def test_readout_recovers_a_planted_mask_exactly(rounding, N, lens, heads, p):
    """``recover_keep`` driven by a plain torch forward with a KNOWN random mask -- exact, and with the probabilities and the context
    rounded to bf16 / fp16 as the 16-bit kernels round them -- returns that mask bit for bit, lengths up to 1000 (16 passes), under the
    decode thresholds the GPU tests use."""
    g = torch.Generator().manual_seed(N + heads)
    B = len(lens)
    planted = torch.rand(B, heads, N, N, generator=g) >= p
    h16 = H16.get(rounding)
    got = helpers.recover_keep(planted_forward(planted, lens, heads, p, h16), B, N, heads, lens, p, tol=DECODE_TOL[rounding or 'f32'])
    assert torch.equal(got, planted & helpers.attention_valid(lens, heads, N))


def test_readout_refuses_what_is_not_a_mask():
    """the helper asserts, it does not assume: a value that is neither 0 nor 1, probability on a key beyond the utterance, a non-zero
    padded query row and a wrong output shape are all refused"""
    N, lens, heads, p = 130, [130, 70], 2, 0.1
    planted = torch.rand(2, heads, N, N, generator=torch.Generator().manual_seed(3)) >= p
    good = planted_forward(planted, lens, heads, p, None)
    helpers.recover_keep(good, 2, N, heads, lens, p)

    def spoiled(edit):
        def fwd(qkv):
            ctx = good(qkv).clone()
            edit(ctx, int(qkv[0, :, 2 * 64 * heads].argmax()) // 64)        # the pass: which key block carries the identity
            return ctx
        return fwd

    def half(ctx, j): ctx[0, 5, 64 + 3] = 0.5 / (130 * 0.9)
    def beyond(ctx, j): ctx[1, 5, 10] += (j == 1) / 70                     # key 64 + 10 = 74 of a 70-token utterance
    def padded(ctx, j): ctx[1, 100, 0] = 1e-3
    for edit in (half, beyond, padded):
        with pytest.raises(AssertionError):
            helpers.recover_keep(spoiled(edit), 2, N, heads, lens, p)
    with pytest.raises(AssertionError):
        helpers.recover_keep(lambda qkv: good(qkv)[:, :, :64], 2, N, heads, lens, p)
    with pytest.raises(AssertionError):                                  # 16-bit rounding is NOT inside the f32 threshold
        helpers.recover_keep(planted_forward(planted, lens, heads, p, torch.bfloat16), 2, N, heads, lens, p, tol=1e-4)


def test_host_mask_is_the_documented_counter():
    """``host_attention_keep`` (vectorised numpy) against the kernels' scalar expressions written out with Python integers:
    drop_index = ((bh N + q) << 16) | key, draw = dx_rand64(seed, drop_index >> 2), field = drop_index & 3, keep = field >= thresh"""
    def rand64(seed, idx):
        m = 0xFFFFFFFF
        x = (idx & m) ^ (seed & m)
        hi = (idx >> 32) ^ (seed >> 32)
        x ^= (hi * 0x9E3779B1) & m
        x ^= x >> 16; x = (x * 0x7FEB352D) & m; x ^= x >> 15; x = (x * 0x846CA68B) & m; x ^= x >> 16
        y = ((x ^ 0x85EBCA6B) * 0xC2B2AE35) & m; y ^= y >> 15
        return (y << 32) | x

    g = torch.Generator().manual_seed(0)
    for seed, B, H, N, p in ((SEED, 3, 2, 150, 0.1), (0xFEDCBA9876543210, 9, 4, 1000, 0.5), (7, 2, 1, 64, 0.25)):
        keep = helpers.host_attention_keep(seed, B, H, N, p)
        assert keep.shape == (B, H, N, N) and keep.dtype == torch.bool
        thresh = int(round(p * 65536))
        picks = torch.stack([torch.randint(0, n, (200,), generator=g) for n in (B, H, N, N)], dim=1).tolist()
        picks += [[B - 1, H - 1, N - 1, N - 1], [0, 0, 0, 0], [B - 1, 0, N - 1, 63], [0, H - 1, 63, 64 % N]]
        for b, h, q, key in picks:
            elem = (((b * H + h) * N + q) << 16) | key
            field = (rand64(seed, elem >> 2) >> (16 * (elem & 3))) & 0xFFFF
            assert bool(keep[b, h, q, key]) == (field >= thresh), (seed, b, h, q, key)
        assert abs(keep.double().mean().item() - (1 - p)) < 6 * math.sqrt(p * (1 - p) / keep.numel())


@pytest.mark.parametrize('p', [0.0, 0.1])
def test_emulation_without_rounding_is_the_float64_reference(p):
    """the reference-only emulation (its own softmax, its own hand-written backward) equals float64 autograd when nothing is rounded:
    whatever it shows with 16-bit rounding is rounding, not a different formula"""
    g = torch.Generator().manual_seed(11)
    B, N, heads, lens = 3, 150, 2, [150, 70, 3]
    qkv, dctx = torch.randn(B, N, 384, generator=g), torch.randn(B, N, 128, generator=g)
    keep = (torch.rand(B, heads, N, N, generator=g) >= p) if p else None
    ref = helpers.attention_reference64(qkv, dctx, lens, heads, keep, p)
    emu = helpers.attention_emulation(qkv, lens, heads, keep, p, None, dctx)
    for name, a, r in zip(('ctx', 'dq', 'dk', 'dv'), emu, (ref[0],) + tuple(ref[2:])):
        assert err(a, r) < 1e-5, (name, err(a, r))
    for b, n in enumerate(lens):
        assert all(not t[b, n:].any() for t in emu)
    e16 = helpers.attention_emulation(qkv, lens, heads, keep, p, torch.bfloat16, dctx)
    assert all(1e-4 < err(a, r) < 3e-2 for a, r in zip(e16, (ref[0],) + tuple(ref[2:])))


# ------------------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ops():
    from ubisoft_laforge_daft_exprt_amd import ops as _ops
    _ops.set_precision('f32')
    return _ops


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


class Case:
    def __init__(self, ops, N, lens, heads=2, p=0.1, ordered=False, strided=False):
        self.ops, self.N, self.lens, self.heads, self.p, self.strided = ops, N, lens, heads, p, strided
        self.B, self.D = len(lens), 64 * heads
        self.ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
        self.order = ops.length_order(self.ln) if ordered else None
        self.valid = (torch.arange(N, device=DEV)[None, :] < self.ln[:, None])[:, :, None]
        self.qkv = randn(self.B, N, 3 * self.D, seed=5)
        self.dctx = randn(self.B, N, self.D, seed=6) * self.valid          # the model never sends gradient into padded queries

    def place(self, t):
        """``t`` as the kernels get it: densely, or as the first 3 D columns of rows 8 elements wider whose tail is NaN"""
        if not self.strided:
            return t.contiguous()
        wide = torch.full((self.B, self.N, 3 * self.D + 8), float('nan'), dtype=t.dtype, device=t.device)
        wide[:, :, :3 * self.D] = t
        return wide[:, :, :3 * self.D]

    def fwd(self, qkv, p, ctx_dtype, seed=SEED, seed_offset=None):
        return self.ops.attention_fwd(qkv, self.ln, self.heads, seed, p, ctx_dtype=ctx_dtype, seed_offset=seed_offset, order=self.order)

    def bwd(self, qkv, ctx, dctx, lse, p, out_dtype, seed=SEED, seed_offset=None):
        return self.ops.attention_bwd(qkv, ctx, dctx, lse, self.ln, self.heads, seed, p, out_dtype=out_dtype, seed_offset=seed_offset,
                                      order=self.order)

    def readout(self, mode, qdt, cdt, seed=SEED, seed_offset=None):
        return helpers.recover_keep(lambda q: self.fwd(self.place(q.to(DEV).to(qdt)), self.p, cdt, seed, seed_offset)[0],
                                    self.B, self.N, self.heads, self.lens, self.p, tol=DECODE_TOL[mode])

    def compare(self, mode, variant, keep, p, tag, seed=SEED, seed_offset=None, emulate=False):
        """forward and backward of one storage variant against float64 under ``keep``; prints every figure, returns the list of misses"""
        name, qdt, cdt, odt = variant
        tol_f, tol_b = BARS[mode]
        qkv = self.place(self.qkv.to(qdt))
        dctx = self.dctx.to(cdt)
        ctx, lse = self.fwd(qkv, p, cdt, seed, seed_offset)
        dqkv = self.bwd(qkv, ctx, dctx, lse, p, odt, seed, seed_offset)
        assert ctx.dtype == cdt and dqkv.dtype == odt and lse.dtype == torch.float32
        lse_is_pre_dropout = torch.equal(lse, self.fwd(qkv, 0.0, cdt)[1])
        ref = helpers.attention_reference64(qkv, dctx, self.ln, self.heads, keep if p else None, p)
        if mode in H16:
            lse = lse * math.log(2.0)                      # the 16-bit kernels keep scores, and so the saved log-sum-exp, in base 2
        got = (ctx, lse) + tuple(dqkv.split(self.D, dim=2))
        names = ('ctx', 'lse', 'dq', 'dk', 'dv')
        figs = {n: err(a, r) for n, a, r in zip(names, got, ref)}
        print(f'[{tag}] {mode} ({name}) p={p}: ' + ' '.join(f'{n}={figs[n]:.2e}' for n in names))
        bad = [(tag, mode, name, p, n, figs[n]) for n in names if not figs[n] < (tol_f if n in ('ctx', 'lse') else tol_b)]
        for b, n_b in enumerate(self.lens):
            if n_b >= 64:
                per = {n: err(a[b], r[b]) for n, a, r in zip(names[2:], got[2:], ref[2:])}
                print(f'[{tag}]     utterance {b} (len {n_b}): ' + ' '.join(f'{n}={per[n]:.2e}' for n in per))
                bad += [(tag, mode, name, p, f'{n}[{b}]', per[n]) for n in per if not per[n] < tol_b]
            if dqkv[b, n_b:].any() or ctx[b, n_b:].any() or lse[b, :, n_b:].any():
                bad.append((tag, mode, name, p, 'padded rows not zero', b))
        if not all(bool(torch.isfinite(t).all()) for t in (ctx, lse, dqkv)):
            bad.append((tag, mode, name, p, 'not finite'))
        if not lse_is_pre_dropout:
            bad.append((tag, mode, name, p, 'lse depends on p'))        # it is taken before the dropout
        if emulate and mode in H16:                         # reference-only: what the mode's rounding alone costs on these inputs
            emu = helpers.attention_emulation(qkv, self.ln, self.heads, keep if p else None, p, H16[mode], dctx)
            emu = (emu[0].to(cdt),) + tuple(t.to(odt) for t in emu[1:])
            print(f'[{tag}]     torch emulation of {mode}: ' + ' '.join(f'{n}={err(a, r):.2e}' for n, a, r in zip(('ctx', 'dq', 'dk', 'dv'), emu, (ref[0],) + ref[2:])))
        return bad


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['f32', 'bf16x3', 'bf16', 'fp16'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_mask_forward_and_each_gradient(ops, shape, mode):
    """Per family and storage variant: the mask read out of the forward is the host mask (so every family and variant draws the same
    one, the contract that lets a forward in one variant pair with a backward in another) and has the binomial keep rate; ctx, lse and
    each of dQ, dK, dV meet the mode's bars against float64 under that mask, over all and per utterance; padded rows are exactly zero;
    everything is finite; lse does not depend on p.  At shape D the read-out runs in f32 and in the all-16-bit variant only (16 passes
    each); the other variants there use the host mask those read-outs are asserted equal to."""
    case = Case(ops, **SHAPES[shape])
    host = helpers.host_attention_keep(SEED, case.B, case.heads, case.N, case.p) & helpers.attention_valid(case.lens, case.heads, case.N)
    ops.set_precision(mode)
    try:
        bad = []
        masks = []
        for variant in variants(mode):
            name, qdt, cdt, odt = variant
            keep = host
            if shape != 'D' or (mode == 'f32') or (mode in H16 and qdt == cdt == H16[mode]):
                keep = case.readout(mode, qdt, cdt)
                masks.append(keep)
                diff = keep ^ host
                if diff.any():
                    where = diff.nonzero()
                    bad.append((shape, mode, name, 'mask differs from the host mask', int(diff.sum()), where[0].tolist(), where[-1].tolist()))
            bad += case.compare(mode, variant, keep.to(DEV), case.p, shape, emulate=True)
            bad += case.compare(mode, variant, None, 0.0, shape, emulate=True)
        assert all(torch.equal(m, masks[0]) for m in masks)
        if masks:
            bad += keep_rate_failures(masks[0], case.lens, case.heads, case.p)
        assert not bad, bad
    finally:
        ops.set_precision('f32')


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['f32', 'bf16x3', 'bf16', 'fp16'])
def test_seed_offset_is_added_to_the_seed(ops, mode):
    """A device int64 ``seed_offset`` o (what a captured graph's replays change): the forward's mask is the one of seed + o without an
    offset, and the backward run with the offset meets the same bars under that mask -- in all three backward kernels' own additions."""
    case = Case(ops, **SHAPES['C'])
    off = 977
    so = torch.tensor([off], dtype=torch.int64, device=DEV)
    ops.set_precision(mode)
    try:
        variant = variants(mode)[-1]
        _, qdt, cdt, _ = variant
        keep = case.readout(mode, qdt, cdt, SEED, so)
        assert torch.equal(keep, case.readout(mode, qdt, cdt, SEED + off, None))
        assert torch.equal(keep, helpers.host_attention_keep(SEED + off, case.B, case.heads, case.N, case.p)
                           & helpers.attention_valid(case.lens, case.heads, case.N))
        assert not torch.equal(keep, case.readout(mode, qdt, cdt, SEED, None))
        bad = case.compare(mode, variant, keep.to(DEV), case.p, 'C+offset', SEED, so)
        assert not bad, bad
    finally:
        ops.set_precision('f32')


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['bf16', 'fp16'])
def test_fused_forward_context_is_the_unfused_one_at_shape_c(ops, mode):
    """dx_attention_proj_ln_fwd's context and lse at shape C, p = 0.1, bitwise those of dx_attention_fwd: the fused kernel's mask and
    forward are thereby covered by the checks above"""
    case = Case(ops, **SHAPES['C'])
    ops.set_precision(mode)
    try:
        h16 = H16[mode]
        qkv = case.qkv.to(h16)
        res = randn(case.B, case.N, 128, seed=2)
        wout, bout = randn(128, 128, seed=3, scale=0.09), randn(128, seed=4, scale=0.1)
        ln_w, ln_b = 1 + randn(128, seed=5, scale=0.1), randn(128, seed=6, scale=0.1)
        pack = ops.PackedWeight(wout)
        assert ops.attn_proj_ln_applies(qkv, 2, pack, mode)
        ctx0, lse0 = case.fwd(qkv, case.p, h16)
        out = ops.attn_proj_ln_fwd(qkv, case.ln, 2, SEED, case.p, pack, bout, res, ln_w, ln_b, None, seed_pre=12, p_pre=0.1)
        assert torch.equal(out[0], ctx0) and torch.equal(out[1], lse0)
    finally:
        ops.set_precision('f32')
