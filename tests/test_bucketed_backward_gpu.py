"""Kernel-level contract of ``rows_exist`` in the backward launches (bucketed training, trainer.Trainer(bucket=...)): a launch given
rows_exist = E on tensors allocated with N > E rows must give, on rows n < E, what the same launch gives on the tensors cut to E rows;
gradient rows n >= E are zero; and nothing stored in rows n >= E of any input reaches a result (those rows hold real halo values of the
longest utterances in a bucketed forward).  Every test below allocates N = E + 17 rows, lengths {E, E - 1, short}, and runs the padded
launch twice: once with the forward's values in rows >= E and once with large finite garbage there."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
E, PAD = 150, 17
N = E + PAD
LENS = [E, E - 1, 61]


@pytest.fixture(scope='module')
def ops():
    from ubisoft_laforge_daft_exprt_amd import ops as _ops
    _ops.set_precision('f32')
    return _ops


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(DEV)


def i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device=DEV)


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max().clamp_min(1e-12)).item()


def garbage(t, seed, axis=1):
    """t with every row n >= E along ``axis`` overwritten by +-1e3 (finite in every storage type)."""
    t = t.clone()
    idx = [slice(None)] * t.dim()
    idx[axis] = slice(E, None)
    sign = torch.where(randn(*t[tuple(idx)].shape, seed=seed) > 0, 1e3, -1e3)
    t[tuple(idx)] = sign.to(t.dtype)
    return t


def cut(t, axis=1):
    idx = [slice(None)] * t.dim()
    idx[axis] = slice(0, E)
    return t[tuple(idx)].contiguous()


def rows_ge(t, axis=1):
    idx = [slice(None)] * t.dim()
    idx[axis] = slice(E, None)
    return t[tuple(idx)]


def halo_values(t, lens, halo, seed, axis=1):
    """t with rows [len, len + halo) of each utterance holding non-zero values, as a k = 3 forward leaves them"""
    t = t.clone()
    for b, n in enumerate(lens):
        idx = [slice(None)] * t.dim()
        idx[0] = b
        idx[axis] = slice(n, min(n + halo, t.shape[axis]))
        v = t[tuple(idx)]
        t[tuple(idx)] = randn(*v.shape, seed=seed + b).to(t.dtype)
    return t


@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('halo', [0, 1, 2])
def test_input_gradient_conv(ops, precision, halo):
    """dx_conv_gemm on the backward pack (dY -> dX, the f32 FFT arm, the prenet, the pitch predictor's layer path): rows < E bitwise as on
    the cut tensors, rows >= E zero, garbage in dY rows >= E never reaches dX; with accumulate, rows >= E of the output are left as they are."""
    ops.set_precision(precision)
    try:
        hd = ops.hidden_dtype(precision)
        B, Cin, Cout = len(LENS), 128, 256
        w = randn(Cout, Cin, 3, seed=1, scale=1 / math.sqrt(3 * Cin))
        pack = ops.PackedWeight(w)
        L = i32(LENS)
        dy = halo_values(randn(B, N, Cout, seed=2) * (torch.arange(N, device=DEV)[None, :, None] < L[:, None, None]), LENS, halo + 1, 50).to(hd)
        aux = randn(B, N, Cout, seed=3).to(hd)
        kw = dict(transpose=True, lens=L, halo=halo, prec=precision, out_dtype=hd)
        ref = ops.conv_gemm(cut(dy), pack, None, relu_aux=cut(aux), **kw)
        ex = i32([E] * B)
        for g in (dy, garbage(dy, 7)):
            out = ops.conv_gemm(g, pack, None, relu_aux=garbage(aux, 8), rows_exist=ex, **kw)
            assert torch.equal(cut(out), ref), rel(cut(out), ref)
            assert float(rows_ge(out).float().abs().max()) == 0.0
        # accumulate (the f32 arm's residual add): rows >= E keep what the output held
        base = randn(B, N, Cin, seed=9)
        acc = base.clone()
        ops.conv_gemm(garbage(dy, 10), pack, None, out=acc, accumulate=True, lens=L, halo=halo, prec=precision, transpose=True, rows_exist=ex)
        accr = cut(base)
        ops.conv_gemm(cut(dy), pack, None, out=accr, accumulate=True, lens=L, halo=halo, prec=precision, transpose=True)
        assert torch.equal(cut(acc), accr) and torch.equal(rows_ge(acc), rows_ge(base))
    finally:
        ops.set_precision('f32')


@pytest.mark.parametrize('precision', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('Cin,Cout,halo,stored16', [(128, 1024, 1, (False, True)), (1024, 128, 0, (True, True)), (80, 1024, 2, (True, False)),
                                                    (1024, 1024, 1, (True, True))])
def test_weight_gradient(ops, precision, Cin, Cout, halo, stored16):
    """dx_conv_wgrad (and the queued dx_conv_wgrad_batched where its shape rules apply): X and dY rows >= E read as zero, so the weight and
    bias gradients equal those of the cut tensors and do not see what rows >= E hold."""
    ops.set_precision(precision)
    try:
        B = len(LENS)
        h16 = ops.hidden_dtype(precision)
        dyt = h16 if stored16[0] and precision != 'f32' else torch.float32
        xt = h16 if stored16[1] and precision != 'f32' else torch.float32
        pack = ops.PackedWeight(randn(Cout, Cin, 3, seed=1, scale=0.05))
        L = i32(LENS)
        valid = (torch.arange(N, device=DEV)[None, :, None] < L[:, None, None])
        x = halo_values(randn(B, N, Cin, seed=2) * valid, LENS, halo + 1, 60).to(xt)        # forward halo rows are real values
        dy = halo_values(randn(B, N, Cout, seed=3) * valid, LENS, halo, 70).to(dyt)
        ref_w, ref_b = ops.conv_wgrad(cut(dy), cut(x), pack, L, halo, prec=precision)
        ex = i32([E] * B)
        tol = 1e-6 if precision == 'f32' else 2e-3
        for gx, gdy in ((x, dy), (garbage(x, 11), garbage(dy, 12))):
            w, b = ops.conv_wgrad(gdy, gx, pack, L, halo, prec=precision, rows_exist=ex)
            assert rel(w, ref_w) <= tol and rel(b, ref_b) <= tol, (rel(w, ref_w), rel(b, ref_b))
            if precision != 'f32' and Cin % 128 == 0:
                rt = ops.DEFAULT
                rt.defer_wgrad = True
                try:
                    gw, gb = torch.zeros_like(pack.weight), torch.zeros(Cout, device=DEV)
                    assert ops.conv_wgrad(gdy, gx, pack, L, halo, w_sink=gw, b_sink=gb, prec=precision, defer=True, rows_exist=ex) == (None, None)
                    assert ops.flush_wgrads(rt) == 1
                finally:
                    rt.defer_wgrad = False
                assert rel(gw, ref_w) <= tol and rel(gb, ref_b) <= tol, (rel(gw, ref_w), rel(gb, ref_b))
    finally:
        ops.set_precision('f32')


def _ff_block_inputs(ops, precision, Bm):
    h16 = ops.hidden_dtype(precision)
    lens = LENS * Bm
    B, Fc = len(lens), 1024
    L = i32(lens)
    valid = (torch.arange(N, device=DEV)[None, :] < L[:, None])
    vf = valid[:, :, None].float()
    p1 = ops.PackedWeight(randn(Fc, 128, 3, seed=2, scale=1 / math.sqrt(384)))
    p2 = ops.PackedWeight(randn(128, Fc, 3, seed=4, scale=1 / math.sqrt(3 * Fc)))
    x = (randn(B, N, 128, seed=1) * vf).to(h16)
    h = ops.conv_gemm(x, p1, randn(Fc, seed=3, scale=0.1), relu=True, lens=L, halo=1, out_dtype=h16, rows_exist=i32([E] * B))
    h = halo_values(h, lens, 2, 80)
    dy2 = randn(B, N, 128, seed=5) * vf
    z2, z1 = randn(B, N, 128, seed=6), randn(B, N, 128, seed=7)
    st = lambda z: (z.mean(dim=2), 1.0 / torch.sqrt(z.var(dim=2, unbiased=False) + 1e-5))
    (m2, r2), (m1, r1) = st(z2), st(z1)
    lnp = (1 + 0.1 * randn(128, seed=8), randn(128, seed=9, scale=0.1), 1 + 0.1 * randn(128, seed=10), randn(128, seed=11, scale=0.1))
    film = randn(B, 256, seed=12)
    po = ops.PackedWeight(randn(128, 128, seed=13, scale=0.09))
    return dict(L=L, B=B, p1=p1, p2=p2, h=h, dy2=dy2, z2=z2, m2=m2, r2=r2, z1=z1, m1=m1, r1=r1, lnp=lnp, film=film, po=po)


def _ff_block(ops, d, rows, p, ex=None, mutate=None):
    c = (lambda t: t) if rows == N else cut
    tens = {k: c(d[k]) for k in ('h', 'dy2', 'z2', 'z1')}
    tens.update({k: c(d[k]) for k in ('m2', 'r2', 'm1', 'r1')})
    if mutate is not None:
        tens = {k: mutate(v, i) for i, (k, v) in enumerate(tens.items())}
    l2w, l2b, l1w, l1b = d['lnp']
    return ops.ff_block_bwd(tens['dy2'], tens['z2'], tens['m2'], tens['r2'], l2w, l2b, d['film'], d['p1'], d['p2'], d['L'], tens['h'],
                            tens['z1'], tens['m1'], tens['r1'], l1w, l1b, seed2=71, p2=p, seed1=72, p1=p, out_pack=d['po'], rows_exist=ex)


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
@pytest.mark.parametrize('Bm', [1, 16])      # 3 / 48 utterances: the 62-token and the 126-token tile forms
def test_fused_ff_block_backward(ops, precision, Bm):
    """dx_ff_block_bwd: dz1, the hidden gradient, both 16-bit gradient copies and the out-projection's input gradient bitwise on rows < E
    and zero on rows >= E; the LayerNorm and FiLM gradients within the 16-bit bar; garbage in rows >= E of every input changes nothing."""
    ops.set_precision(precision)
    try:
        d = _ff_block_inputs(ops, precision, Bm)
        ref = _ff_block(ops, d, E, 0.0)
        ex = i32([E] * d['B'])
        for mut in (None, lambda t, i: garbage(t, 20 + i)):
            out = _ff_block(ops, d, N, 0.0, ex, mut)
            for i in (0, 1, 2, 3, 9):              # dz1, dh, dg1, dg2, datt
                assert torch.equal(cut(out[i]), ref[i]), (i, rel(cut(out[i]), ref[i]))
                assert float(rows_ge(out[i]).float().abs().max()) == 0.0, i
            for i in (4, 5, 6, 7, 8):              # dfilm, the affine gradients
                assert rel(out[i], ref[i]) <= 2e-3, (i, rel(out[i], ref[i]))
    finally:
        ops.set_precision('f32')


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_fused_ff_block_backward_dropout(ops, precision):
    """Dropout on: masks are indexed over the allocated row stride, so the padded launch is compared with itself -- the same launch with
    garbage in rows >= E gives the same results, and rows >= E stay zero."""
    ops.set_precision(precision)
    try:
        d = _ff_block_inputs(ops, precision, 1)
        ex = i32([E] * d['B'])
        a = _ff_block(ops, d, N, 0.2, ex)
        b = _ff_block(ops, d, N, 0.2, ex, lambda t, i: garbage(t, 40 + i))
        for i in (0, 1, 2, 3, 9):
            assert torch.equal(a[i], b[i]), i
            assert float(rows_ge(a[i]).float().abs().max()) == 0.0, i
        for i in (4, 5, 6, 7, 8):
            assert rel(a[i], b[i]) <= 2e-3, i
    finally:
        ops.set_precision('f32')


@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_fused_pitch_predictor_chain(ops, precision):
    """dx_pitch_chain_fwd / _bwd (the loss's frozen pitch predictor, halos 3, 2, 1, 0 over the frame axis): the prediction, the sign words
    of the valid frames and the mel gradient on frames < E equal those of the cut tensors; the mel, dpp and sign words stored at frames
    >= E are ignored."""
    from ubisoft_laforge_daft_exprt_amd import loss as Lo
    ops.set_precision(precision)
    try:
        g = torch.Generator().manual_seed(7)
        state = {}
        for k, shape in Lo.pitch_predictor_shapes().items():
            if k.endswith('num_batches_tracked'):
                state[k] = torch.tensor(10)
            elif k.endswith('running_var') or k.endswith('weight_g'):
                state[k] = torch.rand(shape, generator=g) + 0.5
            else:
                state[k] = torch.randn(shape, generator=g) * (0.3 if 'weight_v' in k else 0.2)
        layers = Lo.fold_pitch_predictor(state, DEV, ops.DEFAULT)
        B, M = len(LENS), 80
        L = i32(LENS)
        valid = (torch.arange(N, device=DEV)[None, :] < L[:, None])
        mel = (randn(B, M, N, seed=3) * valid[:, None, :]).contiguous()
        dpp = (randn(B, N, seed=5) * valid).contiguous()
        pp0, masks0 = ops.pitch_chain_fwd(cut(mel, 2), layers, L, precision)
        dmel0 = torch.zeros(B, M, E, device=DEV)
        ops.pitch_chain_bwd(cut(dpp), masks0, layers, L, precision, dmel0)
        ex = i32([E] * B)
        for gm, gd in ((mel, dpp), (garbage(mel, 30, axis=2), garbage(dpp, 31))):
            pp, masks = ops.pitch_chain_fwd(gm.contiguous(), layers, L, precision, rows_exist=ex)
            assert torch.equal(cut(pp), pp0) and float(rows_ge(pp).abs().max()) == 0.0
            for b, n in enumerate(LENS):             # the sign words of the valid frames (the kernel leaves the others unwritten)
                assert torch.equal(masks[b, :n], masks0[b, :n])
            dmel = torch.zeros(B, M, N, device=DEV)
            ops.pitch_chain_bwd(gd.contiguous(), garbage(masks, 32), layers, L, precision, dmel, rows_exist=ex)
            assert torch.equal(cut(dmel, 2), dmel0) and float(rows_ge(dmel, 2).abs().max()) == 0.0
    finally:
        ops.set_precision('f32')
