"""The LayerNorm row passes, element by element against float64 (tests/ln_exact_helpers.py states the restatement, the host-rebuilt
dropout masks, the inputs and the a-priori bounds; tests/test_ln_exact_cpu.py tests that statement, shows that fp32 evaluations through
each of the four summation trees keep every bound and that the planted faults break them).  The C entries are called directly on buffers
of the test's own: outputs pre-filled with a sentinel, accumulated outputs (dw, dbias, dfilm) on a dyadic base, FiLM rows with a padded
leading dimension.  The backward is handed the mean / rstd given to the kernel; the fused forward launches are restated on the z the
device wrote.  "Equal" in the exact tier means equal as numbers, every element, no tolerance (the sign of a zero is not compared: a
dropped element of a negative gradient is -0 in one summation order and +0 in another).

Measured on the MI355X: the worst ratio of |device - float64| to the bound per output, over the five kinds of input of each path (the z
the LayerNorm gets is: randn; mean 100 with sigma 0.012, the offset riding in the residual - sigma 0.25 / 2 in fp16 / bf16 rows, which
cannot hold less at 100; sigma 1e-4; ReLU'd rows, without FiLM; 1 % outliers x 300); in brackets the same figure from the CPU emulation of that
path's tree (tests/test_ln_exact_cpu.py).  DESIGN.md, "The LayerNorm row passes against float64", has the full table.
  exact backward tier             dz, da, 16-bit copy, dw, dbias, both halves of dfilm equal float64 on all four statements of the
                                  backward (dx_ln_bwd 4 and 16 waves, C = 1024 in fp32 / bf16 / fp16 rows, the pair's epilogue, the block
                                  backward's prologue and the composition of the two), p in {0, 0.5, 0.75}, both builds, both tile widths
  exact forward facts             z and the integer mean bitwise; rstd equal to the correctly rounded fp32 chain in every case (so within
                                  2 ulp of float64); padded rows zero; 16-bit copies = RNE of the fp32 output; constant rows give film(b)
  C = 128, 4 waves, 210 rows      z 0.95   mean 0.21 (0.21)   rstd 0.32 (0.32)   y 0.56 (0.56)   dz 0.33 (0.33)   da 0.34 (0.34)
                                  dw 0.072 (0.098)   dbias 0.030 (0.030)   dfilm 0.15 / 0.077 (0.15 / 0.077)
  C = 128, 16 waves, 16 448 rows  z 0.99   mean 0.33 (0.33)   rstd 0.35 (0.35)   y 0.91 (0.91)   dz 0.48 (0.48)   da 0.47 (0.47)
                                  dw 0.0027 (0.0023)   dbias 0.0012 (0.0016)   dfilm 0.12 / 0.075 (0.12 / 0.075)
  C = 1024 fp32, 32-row blocks    z 0.99   mean 0.062 (0.062)   rstd 0.31 (0.31)   y 0.74 (0.74)   dz 0.36 (0.36)   da 0.34 (0.34)
                                  dw 0.18 (0.18)   dbias 0.026 (0.034)   dfilm 0.17 / 0.087 (0.16 / 0.087)
  the offset rows alone           C = 128 / 16 waves / 1024 fp32: mean 0.11 / 0.15 / 0.062, rstd 0.017 / 0.024 / 0.0039, y 0.12 / 0.16 / 0.065,
                                  dz 0.31 / 0.39 / 0.32;  bf16 / fp16 rows: rstd 0.17 / 0.16
  C = 1024 bf16 / fp16 rows       z = a bit for bit   mean 0.044 / 0.068   rstd 0.29 / 0.30   y, dz, da 0.99 - 1.00 (the 16-bit store's half ulp is the bound);
                                  none of the stored y, dz, da outside [RNE16(ref - fp32 bound), RNE16(ref + fp32 bound)] (lx.between16)
                                  dw 0.14 / 0.13   dbias 0.031 / 0.029   dfilm 0.19 / 0.16
  second grid-stride pass         C = 128: z 0.96, mean 0.036, rstd 0.17, y 0.18;  C = 1024 bf16 / fp16: mean 0.005 / 0.006, rstd 0.11 / 0.12, y 0.99
  dx_proj_ln_fwd, 127 / 129 rows  z 0.097 of the GEMM bound   mean 0.039   rstd 0.16   y 0.18
  dx_ff_pair_ln, 62 / 126 tokens  mean 0.068 / 0.079   rstd 0.21 / 0.24   y 0.20 / 0.59   q_out 0.99 of the GEMM bound (its 16-bit store's half ulp)
The device's ratios are the emulation's to two digits on every per-row output: the kernels round where the restated trees do.  The one
ratio above 1 the device ever showed was the test's: y = 2.5e-5 in fp16 rows, an fp16 subnormal, at 2.08 x a bound that lacked the half
subnormal step (2^-25) the GEMM section already carries; the CPU emulation reproduces 2.08 and the term is now in the bound.  No kernel was
changed.  Wall time of this file on the MI355X: 6.3 s for 74 tests; tests/test_kernels_gpu.py in the same run: 11.4 s for 134.
"""
import math

import pytest
import torch

from tests import gemm_exact_helpers as gx
from tests import ln_exact_helpers as lx

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = lx.SENTINEL
U = lx.U


@pytest.fixture(scope='module')
def lib():
    from ubisoft_laforge_daft_exprt_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def ops():
    from ubisoft_laforge_daft_exprt_amd import ops
    return ops


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


_ALIVE = []       # a launch gets raw pointers: every device copy made for one stays referenced until its test ends


@pytest.fixture(autouse=True)
def _keep_device_copies_alive():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def dev(t):
    _ALIVE.append(t.to(DEV).contiguous())
    return _ALIVE[-1]


def filled(*shape, value=SENTINEL, dtype=torch.float32):
    _ALIVE.append(torch.full(shape, value, dtype=dtype, device=DEV))
    return _ALIVE[-1]


def show(what, **figures):
    print(f'{what}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in figures.items()))


def entry(lib, name, build):
    return getattr(lib, name + ('_f16' if build == 'fp16' else ''))


def same(got, want):
    """equal as numbers, element by element, nothing NaN"""
    got, want = lx.cpu(got, torch.float64), lx.cpu(want, torch.float64)
    return got.shape == want.shape and bool((got == want).all())


def amax(t):
    """largest magnitude of a tensor, 0 for an empty one"""
    return float(t.float().abs().max()) if t.numel() else 0.0


def lens_dev(c):
    return None if c['lens'] is None else dev(torch.tensor(c['lens'], dtype=torch.int32))


def film_dev(c):
    if c['film'] is None:
        return None
    f = filled(c['B'], c['ld_film'])
    f[:, :2 * c['C']] = dev(c['film'])
    return f


def offset_dev(c, use=True):
    return dev(torch.tensor([c['seed_offset']], dtype=torch.int64)) if use else None


def io_dtype(c):
    return lx.H16[c['io16']] if c['io16'] else torch.float32


def valid_mask(c):
    return lx.valid_rows(c, lx.all_rows(c)).reshape(c['B'], c['N'])


# ---- launches -------------------------------------------------------------------------------------------------------------------------
def run_fwd(lib, c, build='bf16', shadow=False, use_offset=True):
    B, N, C = c['B'], c['N'], c['C']
    build = c['io16'] or build
    a = dev(c['a']).clone()
    _ALIVE.append(a)
    y, mean, rstd = filled(B, N, C, dtype=io_dtype(c)), filled(B, N), filled(B, N)
    y_h = filled(B, N, C, dtype=lx.H16[build]) if shadow else None
    add = 0 if use_offset else c['seed_offset']
    entry(lib, 'dx_ln_fwd', build)(P(a), P(None if c['res'] is None else dev(c['res'])), P(dev(c['w'])), P(dev(c['b'])), P(film_dev(c)), c['ld_film'],
                                   P(lens_dev(c)), c['halo'], P(y), P(mean), P(rstd), B, N, C, c['seed_pre'] + add, c['p_pre'],
                                   c['seed_post'] + add, c['p_post'], P(offset_dev(c, use_offset)), int(c['io16'] is not None), P(y_h), S())
    torch.cuda.synchronize()
    return {'z': a, 'y': y, 'mean': mean, 'rstd': rstd, 'y_h': y_h}


def run_bwd(lib, c, z, mean, rstd, build='bf16', want_da=True, shadow=False, use_offset=True):
    """use_offset False: the same seeds without the device scalar (seed + offset handed over as the seed)"""
    B, N, C = c['B'], c['N'], c['C']
    build = c['io16'] or build
    dt = io_dtype(c)
    dz, da = filled(B, N, C, dtype=dt), (filled(B, N, C, dtype=dt) if want_da else None)
    dg = filled(B, N, C, dtype=lx.H16[build]) if shadow else None
    dw, db = dev(c['base_dw']).clone(), dev(c['base_dbias']).clone()
    dfilm = None
    if c['film'] is not None:
        dfilm = filled(B, c['ld_film'])
        dfilm[:, :2 * C] = dev(c['base_dfilm'])
    _ALIVE.extend([dw, db])
    add = 0 if use_offset else c['seed_offset']
    entry(lib, 'dx_ln_bwd', build)(P(dev(c['dy'])), P(dev(z)), P(dev(mean)), P(dev(rstd)), P(dev(c['w'])), P(dev(c['b'])), P(film_dev(c)), c['ld_film'],
                                   P(lens_dev(c)), c['halo'], P(dz), P(da), P(dw), P(db), P(dfilm), c['ld_film'], B, N, C, c['relu_mask'],
                                   c['seed_pre'] + add, c['p_pre'], c['seed_post'] + add, c['p_post'], P(offset_dev(c, use_offset)),
                                   int(c['io16'] is not None), P(dg), S())
    torch.cuda.synchronize()
    out = {'dz': dz, 'da': da, 'dg': dg, 'dw': dw, 'dbias': db}
    if dfilm is not None:
        out.update(dfilm_gamma=dfilm[:, :C], dfilm_beta=dfilm[:, C:2 * C], dfilm_pad=dfilm[:, 2 * C:])
    return out


def assert_exact_backward(c, out, ref, what, build='bf16'):
    C = c['C']
    if out.get('dz') is not None:
        assert same(out['dz'], lx.expected16(c, ref['dz'])), f"{what}: dz {lx.first_difference(out['dz'], lx.expected16(c, ref['dz']))}"
    if out.get('da') is not None:
        assert same(out['da'], lx.expected16(c, ref['da'])), f"{what}: da {lx.first_difference(out['da'], lx.expected16(c, ref['da']))}"
    if out.get('dg') is not None:
        want = lx.rne16(ref['da'].float(), build)
        assert same(out['dg'], want), f"{what}: the 16-bit copy {lx.first_difference(out['dg'], want)}"
    for k in ('dw', 'dbias', 'dfilm_gamma', 'dfilm_beta'):
        if k in ref and k in out:
            assert same(out[k], ref[k]), f'{what}: {k} {lx.first_difference(out[k], ref[k])}'
    if 'dfilm_pad' in out:
        assert bool((out['dfilm_pad'] == SENTINEL).all()), f'{what}: the padding of the dfilm rows was written'


# ---- exact backward tier: dx_ln_bwd -----------------------------------------------------------------------------------------------------
LN_BWD_EXACT = ['c128_w4', 'c128_w16', 'c1024_f32', 'c1024_bf16', 'c1024_fp16']


@pytest.mark.parametrize('p_pre,p_post', lx.EXACT_P)
@pytest.mark.parametrize('name', LN_BWD_EXACT)
def test_exact_backward_tier_is_bitwise(lib, name, p_pre, p_post):
    kw = lx.EXACT_BWD[name]
    assert lx.bwd_waves_rows(kw['B'], kw['N'], kw['C']) == ((16, 192) if name == 'c128_w16' else (4, 32 if kw['C'] == 1024 else 64))
    for film in (True, False):
        c = lx.exact_bwd_case(p_pre=p_pre, p_post=p_post, film=film, **kw)
        ref = lx.ln_backward(c, c['z'], c['mean'], c['rstd'])
        wide = kw['C'] == 128
        variants = [(True, False, True), (False, wide, True), (wide, wide, False)] if name != 'c128_w16' or film else [(True, True, True)]
        for want_da, shadow, use_offset in variants:
            for build in (('bf16', 'fp16') if shadow else ('bf16',)):
                out = run_bwd(lib, c, c['z'], c['mean'], c['rstd'], build, want_da, shadow, use_offset)
                assert_exact_backward(c, out, ref, f'{name} film={film} da={want_da} shadow={shadow} offset scalar={use_offset} {build}', build)


def test_16383_rows_take_four_waves_16384_sixteen_and_the_shared_rows_agree(lib):
    outs = {}
    for name, form in (('c128_16383', (4, 64)), ('c128_16384', (16, 192))):
        kw = lx.EXACT_BWD[name]
        assert lx.bwd_waves_rows(kw['B'], kw['N'], kw['C']) == form
        c = lx.exact_bwd_case(**kw)
        out = run_bwd(lib, c, c['z'], c['mean'], c['rstd'], shadow=True)
        assert_exact_backward(c, out, lx.ln_backward(c, c['z'], c['mean'], c['rstd']), name)
        outs[name] = (c, out)
    (ca, a), (cb, b) = outs['c128_16383'], outs['c128_16384']
    n = ca['N']
    for k in ('z', 'dy', 'mean', 'rstd'):
        cb[k][:, :n] = ca[k]                               # the 16-wave launch on the 4-wave launch's rows (+ one padded row)
    for k in ('w', 'b', 'film', 'base_dw', 'base_dbias', 'base_dfilm', 'seed_pre', 'seed_post', 'seed_offset'):
        cb[k] = ca[k]
    b = run_bwd(lib, cb, cb['z'], cb['mean'], cb['rstd'], shadow=True)
    for k in ('dz', 'da', 'dg'):
        assert lx.bits_equal(a[k], b[k][:, :n]), f'{k} differs between the two forms'
    for k in ('dw', 'dbias', 'dfilm_gamma', 'dfilm_beta'):
        assert lx.bits_equal(a[k], b[k]), f'{k} differs between the two forms'


# ---- exact backward tier: the feed-forward pair's statements ------------------------------------------------------------------------------
def ff_setup(ops, c, build, zero_first=False):
    """packs and the stored activation of an input-gradient pair whose SECOND weight pack is all zero: it adds exactly 0 to the tile"""
    B, N = c['B'], c['N']
    g = torch.Generator().manual_seed(9)
    w2 = torch.zeros(128, 1024, 3) if zero_first else torch.randn(128, 1024, 3, generator=g) / 55
    p1, p2 = ops.PackedWeight(dev(torch.zeros(1024, 128, 3))), ops.PackedWeight(dev(w2))
    _ALIVE.extend([p1, p2])
    aux = dev(torch.randn(B, N, 1024, generator=g).to(lx.H16[build]))
    return p2.image(build).bwd, p1.image(build).bwd, aux, filled(B, N, 1024, dtype=lx.H16[build])


def ff_live(c):
    """(B, N) bool: rows in a token tile that starts below min(len + 1, N): the tiles the pair computes (skip_halo = 1)"""
    tok = lx.ff_pair_tok(c['B'], c['N'])
    lim = (torch.tensor(c['lens']) + 1).clamp(max=c['N'])
    return (torch.arange(c['N'])[None, :] // tok) < ((lim + tok - 1) // tok)[:, None]


FF = [('bf16', 'ff_62'), ('fp16', 'ff_62'), ('bf16', 'ff_126'), ('fp16', 'ff_126')]


def ff_case(name, p_pre, film=False, seed=0):
    c = lx.exact_bwd_case(p_pre=p_pre, p_post=0.0, film=film, seed=seed, **lx.EXACT_BWD[name])
    c['ld_film'] = 256 + 4
    assert lx.ff_pair_tok(c['B'], c['N']) == (62 if name == 'ff_62' else 126)
    return c


@pytest.mark.parametrize('p_pre', [0.5, 0.0])
@pytest.mark.parametrize('build,name', FF)
def test_exact_tier_through_the_pair_epilogue(lib, ops, build, name, p_pre):
    """dx_ff_pair_lnbwd with an all-zero second pack: the epilogue sees d = the residual gradient already in Y"""
    c = ff_case(name, p_pre)
    B, N = c['B'], c['N']
    ref = lx.ln_backward(c, c['z'], c['mean'], c['rstd'])
    wa, wb, aux, dh = ff_setup(ops, c, build)
    valid, live = valid_mask(c), ff_live(c)
    y = torch.where(valid[:, :, None], torch.nan_to_num(c['dy']), torch.full((), SENTINEL))
    Y, dg = dev(y).clone(), filled(B, N, 128, dtype=lx.H16[build])
    dw, db = dev(c['base_dw']).clone(), dev(c['base_dbias']).clone()
    _ALIVE.extend([Y, dw, db])
    x = dev(torch.randn(B, N, 128, generator=torch.Generator().manual_seed(4)).to(lx.H16[build]))
    entry(lib, 'dx_ff_pair_lnbwd', build)(P(x), 128, P(wa), P(wb), P(aux), 1024, P(dh), 1024, P(Y), B, N, 1024, P(lens_dev(c)), 1,
                                          P(dev(c['z'])), P(dev(c['mean'])), P(dev(c['rstd'])), P(dev(c['w'])), P(dev(c['b'])), P(dg), P(dw), P(db),
                                          c['seed_pre'], c['p_pre'], P(offset_dev(c)), S())
    torch.cuda.synchronize()
    want = torch.where(live[:, :, None], ref['dz'].float(), torch.full((), SENTINEL))      # tiles beyond the halo keep what Y held
    assert same(Y, want), f'dz1 {lx.first_difference(Y, want)}'
    assert_exact_backward(c, {'dz': Y.cpu()[live], 'dg': dg, 'dw': dw, 'dbias': db}, {**ref, 'dz': ref['dz'][live]}, f'{name} {build}', build)


def block_bwd(lib, build, c2, c1, wa, wb, aux, dh, use_film=True):
    B, N = c2['B'], c2['N']
    Y = filled(B, N, 128)
    dg1, dg2 = filled(B, N, 128, dtype=lx.H16[build]), filled(B, N, 128, dtype=lx.H16[build])
    acc = {k: dev(c[f'base_{q}']).clone() for k, c, q in (('dw2', c2, 'dw'), ('db2', c2, 'dbias'), ('dw1', c1, 'dw'), ('db1', c1, 'dbias'))}
    dfilm = None
    if use_film:
        dfilm = filled(B, c2['ld_film'])
        dfilm[:, :256] = dev(c2['base_dfilm'])
    _ALIVE.extend(acc.values())
    assert c1['seed_offset'] == c2['seed_offset']
    entry(lib, 'dx_ff_block_bwd', build)(P(dev(c2['dy'])), P(dev(c2['z'])), P(dev(c2['mean'])), P(dev(c2['rstd'])), P(dev(c2['w'])), P(dev(c2['b'])),
                                         P(film_dev(c2) if use_film else None), c2['ld_film'], P(dg2), P(acc['dw2']), P(acc['db2']), P(dfilm), c2['ld_film'],
                                         c2['seed_pre'], c2['p_pre'], P(wa), P(wb), P(aux), 1024, P(dh), 1024, P(Y), B, N, 1024, P(lens_dev(c2)), 1,
                                         P(dev(c1['z'])), P(dev(c1['mean'])), P(dev(c1['rstd'])), P(dev(c1['w'])), P(dev(c1['b'])), P(dg1), P(acc['dw1']),
                                         P(acc['db1']), c1['seed_pre'], c1['p_pre'], None, None, P(offset_dev(c2)), None, None, S())
    torch.cuda.synchronize()
    out = dict(acc, Y=Y, dg1=dg1, dg2=dg2)
    if dfilm is not None:
        out.update(dfilm_gamma=dfilm[:, :128], dfilm_beta=dfilm[:, 128:256], dfilm_pad=dfilm[:, 256:])
    return out


@pytest.mark.parametrize('p', [0.5, 0.0])
@pytest.mark.parametrize('build,name', FF)
def test_exact_tier_through_the_block_backward(lib, ops, build, name, p):
    """dx_ff_block_bwd with zero packs.  The prologue's dg2 (the dropped-out 16-bit copy of dz2), dw2, db2 and dfilm are direct outputs of
    the second LayerNorm's backward on general exact inputs.  dz1 composes the two backwards: its stage-two rows are constant rows
    (z2 = mean2, so xh = 0) whose dy2 is fixed up until sum(g) is a multiple of 32, which keeps dz2 = rstd2 (g - mean(g)) short enough
    for the first LayerNorm's backward of it to stay exact as well (asserted on the host, intermediate by intermediate)."""
    c2 = ff_case(name, p, film=True, seed=1)
    c1 = ff_case(name, p, film=False, seed=2)
    c1['seed_offset'] = c2['seed_offset']
    wa, wb, aux, dh = ff_setup(ops, c2, build, zero_first=True)
    live = ff_live(c2)
    # (a) the prologue's direct outputs on general inputs
    out = block_bwd(lib, build, c2, c1, wa, wb, aux, dh)
    ref2 = lx.ln_backward(c2, c2['z'], c2['mean'], c2['rstd'])
    got = {'dg': out['dg2'], 'dw': out['dw2'], 'dbias': out['db2'], **{k: out[k] for k in ('dfilm_gamma', 'dfilm_beta', 'dfilm_pad')}}
    assert_exact_backward(c2, got, ref2, f'prologue {name} {build} p={p}', build)
    # (b) the composition on constant stage-two rows
    valid = valid_mask(c2)
    c2['z'] = torch.where(valid[:, :, None], c2['mean'][:, :, None].expand_as(c2['z']), c2['z']).contiguous()
    c2['w'][0], c2['film'][:, 0] = 0.5, 1.0
    g = torch.nan_to_num(c2['dy']).double() * c2['film'][:, None, :128].double() * c2['w'].double()
    c2['dy'][:, :, 0] -= ((g.sum(-1) % 32) / 0.5).float()
    ar = lx.Arith()
    ar.trace = {}
    ref2 = lx.ln_backward(c2, c2['z'], c2['mean'], c2['rstd'], ar)
    c1['dy'] = ref2['dz'].float()
    ref1 = lx.ln_backward(c1, c1['z'], c1['mean'], c1['rstd'], ar)
    assert lx.representable(ref2['dz']) and all(lx.representable(v) and (t is None or lx.order_free(*t)) for recs in ar.trace.values() for v, t in recs)
    out = block_bwd(lib, build, c2, c1, wa, wb, aux, dh)
    want = torch.where(valid[:, :, None], ref1['dz'].float(), torch.zeros(()))           # every row of Y is written: zeros beyond the lengths
    assert same(out['Y'], want), f"dz1 {lx.first_difference(out['Y'], want)}"
    assert_exact_backward(c1, {'dz': out['Y'], 'dg': out['dg1'], 'dw': out['dw1'], 'dbias': out['db1']}, ref1, f'composition {name} {build} p={p}', build)
    assert same(out['dg2'], lx.rne16(ref2['da'].float(), build)) and same(out['dw2'], ref2['dw']) and same(out['dfilm_gamma'], ref2['dfilm_gamma'])
    assert amax(dh.float()) == 0 and bool(live.any())


# ---- exact forward facts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [128, 1024])
def test_exact_forward_facts(lib, C):
    lens = [20, 7, 1, 0]
    record = {}
    for p_pre, res in ((0.5, True), (0.75, True), (0.0, False)):
        c = lx.exact_fwd_case(4, 20, C, lens, halo=1, p_pre=p_pre, res=res)
        rows = lx.all_rows(c)
        valid = valid_mask(c)
        z64, _ = lx.make_z(c, rows)
        ref = lx.ln_stage(c, rows, z64)
        for build in ('bf16', 'fp16'):
            out = run_fwd(lib, c, build, shadow=C == 128)
            # z: bitwise; padded rows of a: zeros where z is stored (residual or pre-dropout), else left as they were
            assert same(out['z'], z64.reshape(c['a'].shape)), f"z {lx.first_difference(out['z'], z64.reshape(c['a'].shape))}"
            if res:
                assert amax(out['z'].cpu()[~valid]) == 0
            else:
                assert lx.bits_equal(out['z'].cpu()[~valid], c['a'][~valid])
            assert same(out['mean'], ref['mean'].reshape(valid.shape)), 'the mean of integer rows whose sum is a multiple of C is not exact'
            rs, rs64 = out['rstd'].cpu().reshape(-1), ref['rstd']
            ulp = torch.tensor([math.ulp(float(v)) * 2 ** 29 for v in rs64.float()]).double()          # one fp32 ulp of each rstd
            assert bool(((rs.double() - rs64).abs() <= 2 * ulp)[valid.reshape(-1)].all()), 'rstd is more than 2 ulp from float64'
            record[(p_pre, build)] = bool(torch.equal(rs[valid.reshape(-1)], lx.correctly_rounded_rstd(z64)[valid.reshape(-1)]))
            for k in ('y', 'mean', 'rstd') + (('y_h',) if C == 128 else ()):
                assert amax(out[k].cpu()[~valid].float()) == 0, f'{k} of a padded row is not zero'
            if C == 128:
                assert lx.bits_equal(out['y_h'], lx.rne16(out['y'], build)), 'the 16-bit copy is not the RNE rounding of the fp32 y that was written'
    show(f'C = {C}: rstd equals the correctly rounded fp32 chain', **{f'p{p} {b}': v for (p, b), v in record.items()})
    # constant dyadic rows: y = film(drop_post(b)) exactly
    c = lx.exact_fwd_case(4, 20, C, lens, halo=1, p_pre=0.0, res=False)
    c['a'] = (torch.randint(-8, 9, (4, 20, 1), generator=torch.Generator().manual_seed(2)).float() / 4).expand(4, 20, C).contiguous()
    c['p_post'] = 0.5
    out = run_fwd(lib, c)
    valid = valid_mask(c)
    t = c['b'].double() * lx.keep_factors(c['seed_post'], c['seed_offset'], lx.all_rows(c).numpy(), C, 0.5).reshape(4, 20, C)
    want = (c['film'][:, None, :C].double() * t + c['film'][:, None, C:].double()) * valid[:, :, None]
    assert same(out['y'], want), f"constant rows: y {lx.first_difference(out['y'], want)}"
    assert same(out['mean'], c['a'][:, :, 0] * valid)


# ---- rounded tier: dx_ln_fwd and dx_ln_bwd --------------------------------------------------------------------------------------------------
def check_stage(c, rows, out, n, what, store16=None, y_key='y'):
    """mean, rstd, y of the listed rows against the stage restated in float64 on the z the device wrote"""
    C = c['C']
    rows = torch.as_tensor(rows)
    z_dev = out['z'].reshape(-1, C)[rows.to(out['z'].device)].cpu().float()
    ref, bound = lx.ln_stage(c, rows, z_dev.double()), lx.stage_bounds(c, rows, z_dev, n, store16)
    r = {}
    for k in ('mean', 'rstd', 'y'):
        got = out[y_key if k == 'y' else k].reshape(-1, C)[rows.to(DEV)] if k == 'y' else out[k].reshape(-1)[rows.to(DEV)]
        r[k], at = lx.worst_ratio(got, ref[k], bound[k])
        assert r[k] <= 1, f'{what}: {k} is {r[k]:.3g} x its bound at {at} of the checked rows'
        if k == 'y' and store16:
            outside = lx.between16(got, ref[k], lx.stage_bounds(c, rows, z_dev, n)['y'], store16)
            assert outside == 0, f'{what}: {outside} stored y lie outside the roundings of the fp32 bound'
    return r


@pytest.mark.parametrize('kind', lx.KINDS)
@pytest.mark.parametrize('shape', list(lx.SHAPES))
def test_rounded_tier_forward_and_backward(lib, shape, kind):
    c = lx.rounded_case(kind, **lx.SHAPES[shape])
    B, N, C = c['B'], c['N'], c['C']
    n = lx.TREE_N[('rowvec', C)]
    rows = lx.all_rows(c)
    valid = valid_mask(c)
    assert lx.bwd_waves_rows(B, N, C) == ((16, 192) if shape == 'big' else (4, 32 if C == 1024 else 64)) and lx.ln_plan(B, N, C).passes == 1
    out = run_fwd(lib, c, shadow=C == 128)
    z64, _ = lx.make_z(c, rows)
    r = {}
    r['z'], at = lx.worst_ratio(out['z'].reshape(-1, C), z64, lx.z_bound(c, rows))
    assert r['z'] <= 1, f'z is {r["z"]:.3g} x its bound at {at}'
    if c['io16']:                                         # handed over as z: nothing is stored, padded rows included
        assert lx.bits_equal(out['z'], c['a']), 'a was rewritten although there is neither a residual nor a pre-dropout'
    r.update(check_stage(c, rows, out, n, f'{shape} {kind}', c['io16']))
    for k in ('y', 'mean', 'rstd'):
        assert amax(out[k].cpu()[~valid].float()) == 0, f'{k} of a padded row is not zero'
    if C == 128:
        assert lx.bits_equal(out['y_h'], lx.rne16(out['y'], 'bf16'))
    # backward, handed the device's own z, mean, rstd
    z, mean, rstd = out['z'].cpu(), out['mean'].cpu(), out['rstd'].cpu()
    bw = run_bwd(lib, c, z, mean, rstd, shadow=C == 128)
    ref, bound = lx.ln_backward(c, z, mean, rstd), lx.backward_bounds(c, z, mean, rstd, n)
    assert (c['film'] is None) == (kind == 'relu') and ('dfilm_gamma' in ref) == (c['film'] is not None)      # FILM = false: the ReLU'd rows
    for k in ref:
        r[k], at = lx.worst_ratio(bw[k], ref[k], bound[k])
        assert r[k] <= 1, f'{shape} {kind}: {k} is {r[k]:.3g} x its bound at {at}'
    if c['io16']:
        b32 = lx.backward_bounds(c, z, mean, rstd, n, store=False)
        for k in ('dz', 'da'):
            outside = lx.between16(bw[k], ref[k], b32[k], c['io16'])
            assert outside == 0, f'{shape} {kind}: {outside} stored {k} lie outside the roundings of the fp32 bound'
    assert amax(bw['dz'].cpu()[~valid].float()) == 0 and (c['film'] is None or bool((bw['dfilm_pad'] == SENTINEL).all()))
    if C == 128:
        da32 = bw['dz'].cpu() * lx.keep_factors(c['seed_pre'], c['seed_offset'], rows.numpy(), C, c['p_pre']).float().reshape(B, N, C) if c['p_pre'] else bw['dz'].cpu()
        assert lx.bits_equal(bw['da'], da32) and lx.bits_equal(bw['dg'], lx.rne16(da32, 'bf16')), 'da / its 16-bit copy are not dz x the host mask'
    show(f'{shape} {kind}', **r)


@pytest.mark.parametrize('C,io16', [(128, None), (1024, 'bf16'), (1024, 'fp16')])
def test_forward_grid_stride_second_pass(lib, C, io16):
    B, N = lx.WRAP['B'], lx.WRAP['N']
    total = B * N
    assert lx.ln_plan(B, N, C).sweep == 32768 < total and lx.ln_plan(B, N, C).passes == 2      # row_grid's cap: a second pass
    c = lx.rounded_case('randn', C=C, lens=lx.wrap_lens(), io16=io16, with_dy=False, **lx.WRAP)
    out = run_fwd(lib, c)
    rows = lx.wrap_rows()
    assert int((rows >= 32768).sum()) == total - 32768
    z64, _ = lx.make_z(c, rows)
    r = {'z': lx.worst_ratio(out['z'].reshape(-1, C)[rows.to(DEV)], z64, lx.z_bound(c, rows))[0]}
    assert r['z'] <= 1
    r.update(check_stage(c, rows, out, lx.TREE_N[('rowvec', C)], f'wrap C={C}', io16))
    valid = valid_mask(c).to(DEV)
    for k in ('y', 'mean', 'rstd'):
        assert amax(out[k][~valid].float()) == 0, f'{k} of a padded row is not zero'
        assert not bool((out[k][valid].float() == SENTINEL).any()), f'a computed row of {k} was not written'
    if io16:                                              # no residual, no pre-dropout: a is left as it was, padded rows included
        assert lx.bits_equal(out['z'], c['a'])
    else:
        assert amax(out['z'][~valid]) == 0
    show(f'wrap C={C} {io16 or "f32"}', **r)


# ---- rounded tier: the fused forward launches -------------------------------------------------------------------------------------------------
def gemm64(x16, w, bias, build):
    """(y64, S) of x W^T + bias on the operands the device multiplies"""
    w64 = w.to(lx.H16[build]).double()
    x64 = x16.double()
    return x64 @ w64.T + bias.double(), x64.abs() @ w64.abs().T + bias.double().abs()


@pytest.mark.parametrize('B,N', [(3, 43), (1, 127)])            # 129 and 127 rows: 64 k + 1 and 64 k - 1
@pytest.mark.parametrize('build', ['bf16', 'fp16'])
def test_out_projection_layernorm_launch(lib, ops, build, B, N):
    assert (B * N) % 64 in (1, 63)
    c = lx.rounded_case('randn', B, N, 128, [N - 3] if B == 1 else [N, N - 3, 1], with_dy=False)
    c['p_post'] = 0.0
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, N, 128, generator=g).to(lx.H16[build])
    w, pb = torch.randn(128, 128, generator=g) * 0.09, 0.1 * torch.randn(128, generator=g)
    pack = ops.PackedWeight(dev(w))
    z, y, mean, rstd, y_h = filled(B, N, 128), filled(B, N, 128), filled(B, N), filled(B, N), filled(B, N, 128, dtype=lx.H16[build])
    entry(lib, 'dx_proj_ln_fwd', build)(P(dev(x)), 128, P(pack.image(build).fwd), P(dev(pb)), P(z), P(dev(c['res'])), P(dev(c['w'])), P(dev(c['b'])),
                                        P(film_dev(c)), c['ld_film'], P(lens_dev(c)), 0, P(y), P(mean), P(rstd), B, N, c['seed_pre'], c['p_pre'],
                                        P(offset_dev(c)), P(y_h), S())
    torch.cuda.synchronize()
    rows = lx.all_rows(c)
    valid = valid_mask(c)
    a64, S_ = gemm64(x, w, pb, build)
    f = lx.keep_factors(c['seed_pre'], c['seed_offset'], rows.numpy(), 128, c['p_pre']).reshape(B, N, 128)
    z64 = (a64 * f + c['res'].double()) * valid[:, :, None]
    bz = (gx.Q0 * S_ * f + U * (a64 * f).abs() + U * z64.abs()) * valid[:, :, None]
    r = {'z': lx.worst_ratio(z, z64, bz)[0]}
    assert r['z'] <= 1, f'z is {r["z"]:.3g} x the GEMM bound'
    out = {'z': z, 'y': y, 'mean': mean, 'rstd': rstd}
    r.update(check_stage(c, rows, out, lx.TREE_N[('rowvec', 128)], f'proj_ln {build}'))
    for k, t in out.items():
        assert amax(t.cpu()[~valid]) == 0, f'{k} of a padded row is not zero'
    assert lx.bits_equal(y_h, lx.rne16(y, build))
    show(f'proj_ln {build} rows={B * N}', **r)


@pytest.mark.parametrize('with_qkv', [False, True])
@pytest.mark.parametrize('build,name', FF)
def test_pair_forward_layernorm_epilogue(lib, ops, build, name, with_qkv):
    kw = lx.EXACT_BWD[name]
    B, N, lens = kw['B'], kw['N'], kw['lens']
    c = lx.rounded_case('randn', B, N, 128, lens, with_dy=False)
    c['p_post'] = 0.0
    c['ld_film'] = 260
    assert lx.ff_pair_tok(B, N) == (62 if name == 'ff_62' else 126)
    g = torch.Generator().manual_seed(8)
    r_ = lambda *s: torch.randn(*s, generator=g)
    valid = valid_mask(c)
    x = (r_(B, N, 128) * valid[:, :, None]).to(lx.H16[build])
    p1, p2 = ops.PackedWeight(dev(r_(1024, 128, 3) / math.sqrt(384))), ops.PackedWeight(dev(r_(128, 1024, 3) / math.sqrt(3072)))
    wq, bq = r_(384, 128) * 0.09, 0.1 * r_(384)
    pq = ops.PackedWeight(dev(wq))
    _ALIVE.extend([p1, p2, pq])
    z, y, mean, rstd = filled(B, N, 128), filled(B, N, 128), filled(B, N), filled(B, N)
    h, qkv = filled(B, N, 1024, dtype=lx.H16[build]), filled(B, N, 384, dtype=lx.H16[build])
    head = (P(dev(x)), 128, P(p1.image(build).fwd), P(p2.image(build).fwd), P(dev(0.1 * r_(1024))), P(dev(0.1 * r_(128))), P(h), 1024, P(z), B, N, 1024,
            P(lens_dev(c)), 1, None, P(dev(c['res'] * valid[:, :, None])), P(dev(c['w'])), P(dev(c['b'])), P(film_dev(c)), c['ld_film'], P(y), P(mean), P(rstd),
            c['seed_pre'], c['p_pre'], P(offset_dev(c)))
    if with_qkv:
        entry(lib, 'dx_ff_pair_ln_qkv', build)(*head, P(pq.image(build).fwd), P(dev(bq)), P(qkv), None, S())
    else:
        entry(lib, 'dx_ff_pair_ln', build)(*head, None, S())
    torch.cuda.synchronize()
    live = ff_live(c)
    rows = lx.all_rows(c)[live.reshape(-1)]                # mean / rstd exist in the tiles the pair computes
    out = {'z': z, 'y': y, 'mean': mean, 'rstd': rstd}
    r = check_stage(c, rows, out, lx.TREE_N[('pair32', 128)], f'ff_pair_ln {name} {build}')
    assert amax(z.cpu()[~valid]) == 0 and amax(y.cpu()[~valid]) == 0
    assert amax(mean.cpu()[live & ~valid]) == 0 and amax(rstd.cpu()[live & ~valid]) == 0
    assert bool((mean.cpu()[~live] == SENTINEL).all()) and bool((rstd.cpu()[~live] == SENTINEL).all())       # tiles beyond the halo: not written
    if with_qkv:
        q64, S_ = gemm64(lx.rne16(y, build), wq, bq, build)
        bound = gx.Q0 * S_ + gx.U_H[build] * q64.abs() + (2.0 ** -25 if build == 'fp16' else 0.0)
        r['qkv'], at = lx.worst_ratio(qkv.cpu()[valid], q64[valid], bound[valid])
        assert r['qkv'] <= 1, f'q_out is {r["qkv"]:.3g} x the GEMM bound at {at}'
        assert amax(qkv.cpu()[~live].float()) == 0
    show(f'ff_pair_ln{"_qkv" if with_qkv else ""} {name} {build}', **r)
