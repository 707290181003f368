"""tests/ln_exact_helpers.py tested on the CPU: the float64 restatement of the LayerNorm family against torch.nn.functional.layer_norm +
autograd, the a-priori bounds against fp32 evaluations (plain fp32 torch and an emulation of each of the four summation trees, with and
without fma contraction) on every input of the GPU test's rounded tier, the planted faults against the same bounds, and the exact tier's
claim that every intermediate is an fp32 number.  Run with -s for the worst ratios ("The LayerNorm row passes against float64")."""
import pytest
import torch
import torch.nn.functional as F

from tests import ln_exact_helpers as lx


def show(what, **figures):
    print(f'{what}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in figures.items()))


# ---- the restatement against torch --------------------------------------------------------------------------------------------------
OPTIONS = [dict(), dict(film=False), dict(io16='bf16'), dict(kind='relu'), dict(lens=None), dict(halo=2), dict(C=1024, halo=2),
           dict(C=1024, film=False, kind='relu')]


@pytest.mark.parametrize('opt', OPTIONS, ids=lambda o: '-'.join(f'{k}={v}' for k, v in o.items()) or 'default')
def test_restatement_equals_torch_layer_norm_and_autograd(opt):
    kw = dict(kind='randn', B=3, N=9, C=128, lens=[9, 5, 1])
    kw.update(opt)
    if kw.get('io16'):
        kw['C'] = 1024
    c = lx.rounded_case(**kw)
    B, N, C = c['B'], c['N'], c['C']
    rows = lx.all_rows(c)
    valid = lx.valid_rows(c, rows)
    a = c['a'].double().reshape(-1, C).requires_grad_(True)
    w, b = c['w'].double().requires_grad_(True), c['b'].double().requires_grad_(True)
    film = None if c['film'] is None else c['film'].double().requires_grad_(True)
    z = torch.relu(a) if c["relu_mask"] else a         # the ReLU'd rows: the kernel is handed z = relu(a) and masks by z > 0
    if c['p_pre']:
        z = z * lx.keep_factors(c['seed_pre'], c['seed_offset'], rows.numpy(), C, c['p_pre'])
    if c['res'] is not None:
        z = z + c['res'].double().reshape(-1, C)
    y = F.layer_norm(z, (C,), w, b, eps=lx.EPS)
    if c['p_post']:
        y = y * lx.keep_factors(c['seed_post'], c['seed_offset'], rows.numpy(), C, c['p_post'])
    if film is not None:
        bi = rows // N
        y = film[bi, :C] * y + film[bi, C:]
    y = y * valid[:, None]
    (y * c['dy'].double().reshape(-1, C)).sum().backward()

    z64, _ = lx.make_z(c, rows)
    st = lx.ln_stage(c, rows, z64)
    close = lambda got, want: float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-300)
    assert close(z64[valid], z.detach()[valid]) and close(st['y'], y.detach())
    assert close(st['mean'][valid], z.detach().mean(-1)[valid])
    assert close(st['rstd'][valid], 1 / torch.sqrt(z.detach().var(-1, unbiased=False) + lx.EPS)[valid])
    zero = {k: torch.zeros_like(c[k]) for k in ('base_dw', 'base_dbias', 'base_dfilm')}
    bw = lx.ln_backward({**c, **zero}, z64, st['mean'], st['rstd'])
    assert close(bw['da'].reshape(-1, C), a.grad) and close(bw['dw'], w.grad) and close(bw['dbias'], b.grad)
    if film is not None:
        assert close(torch.cat([bw['dfilm_gamma'], bw['dfilm_beta']], 1), film.grad)


@pytest.mark.parametrize('shape', list(lx.SHAPES))
def test_every_kind_of_input_is_what_its_name_says(shape):
    """the z the LayerNorm stage is handed, after the pre-dropout and the residual: mean and standard deviation of every computed row"""
    for kind in lx.KINDS:
        c = lx.rounded_case(kind, **lx.SHAPES[shape])
        rows = lx.all_rows(c)
        z = lx.make_z(c, rows)[0][lx.valid_rows(c, rows)]
        if c['io16']:
            assert lx.representable(z, lx.H16[c['io16']])
        (m_lo, m_hi), (s_lo, s_hi) = lx.kind_stats(c)
        mean, std = z.mean(-1), z.var(-1, unbiased=False).sqrt()
        show(f'{shape} {kind}', mean_min=float(mean.min()), mean_max=float(mean.max()), std_min=float(std.min()), std_max=float(std.max()))
        assert m_lo <= float(mean.min()) and float(mean.max()) <= m_hi, f'{shape} {kind}: row means {float(mean.min()):.4g} .. {float(mean.max()):.4g}'
        assert s_lo <= float(std.min()) and float(std.max()) <= s_hi, f'{shape} {kind}: row sigmas {float(std.min()):.4g} .. {float(std.max()):.4g}'
        if kind == 'relu':
            assert 0.3 < float((z == 0).double().mean()) < 0.7 and c['film'] is None
        if kind == 'outlier':
            assert float(z.abs().max()) > 300


def test_launch_rules_restated():
    """asked of the library's own plans (dx_ln_plan, dx_ff_pair_plan): a changed threshold in csrc/ fails here"""
    assert lx.bwd_waves_rows(64, 257, 128) == (16, 192) and lx.bwd_waves_rows(1, 16383, 128) == (4, 64) and lx.bwd_waves_rows(1, 16384, 128) == (16, 192)
    assert lx.bwd_waves_rows(64, 257, 1024) == (4, 32)
    for C in (128, 1024):
        assert lx.ln_plan(1, 40000, C).sweep == 32768 and lx.ln_plan(1, 32768, C).passes == 1 and lx.ln_plan(lx.WRAP['B'], lx.WRAP['N'], C).passes == 2
    assert lx.ff_pair_tok(5, 300) == 62 and lx.ff_pair_tok(35, 300) == 126
    assert lx.thresh(0.1) == 6554 and lx.thresh(0.5) == 32768 and lx.inv_keep(0.75) == 4.0


def test_host_masks_keep_the_documented_share():
    f = lx.keep_factors(5, 2, range(400), 128, 0.2)
    assert abs(float((f > 0).double().mean()) - 0.8) < 0.01 and set(f.unique().tolist()) == {0.0, lx.inv_keep(0.2)}
    assert torch.equal(f, lx.keep_factors(7, 0, range(400), 128, 0.2)) and not torch.equal(f, lx.keep_factors(6, 0, range(400), 128, 0.2))


# ---- fp32 evaluations against the bounds ----------------------------------------------------------------------------------------------
def evaluate(c, ar, n):
    """worst ratios of an fp32 evaluation: the stage on its own fp32 z, the backward on its own fp32 mean / rstd (the hand-off rule)"""
    rows = lx.all_rows(c)
    z32, _ = lx.make_z(c, rows, ar)
    z64, _ = lx.make_z(c, rows)
    r = {'z': lx.worst_ratio(z32, z64, lx.z_bound(c, rows))[0]}
    got, ref, bound = lx.ln_stage(c, rows, z32, ar), lx.ln_stage(c, rows, z32.double()), lx.stage_bounds(c, rows, z32, n, c['io16'])
    if c['io16']:
        got['y'] = got['y'].to(lx.H16[c['io16']])
        z32 = z32.to(lx.H16[c['io16']])              # the backward reads the stored z
    for k in ('mean', 'rstd', 'y'):
        r[k] = lx.worst_ratio(got[k], ref[k], bound[k])[0]
    if c['io16']:
        r['y16'] = lx.between16(got['y'], ref['y'], lx.stage_bounds(c, rows, z32, n)['y'], c['io16'])
    if ar.fault is not None:                            # a faulty backward is handed what a sound forward leaves
        clean = lx.Arith(ar.dtype, ar.tree, ar.use_fma)
        z32 = lx.make_z(c, rows, clean)[0]
        got = lx.ln_stage(c, rows, z32, clean)
        z32 = z32.to(lx.H16[c['io16']]) if c['io16'] else z32
    bw, bw64 = lx.ln_backward(c, z32, got['mean'], got['rstd'], ar), lx.ln_backward(c, z32.double(), got['mean'], got['rstd'])
    bb = lx.backward_bounds(c, z32, got['mean'], got['rstd'], n)
    bb32 = lx.backward_bounds(c, z32, got['mean'], got['rstd'], n, store=False) if c['io16'] else None
    for k in bw:
        v = bw[k].to(lx.H16[c['io16']]) if c['io16'] and k in ('dz', 'da') else bw[k]
        r[k] = lx.worst_ratio(v, bw64[k], bb[k])[0]
        if c['io16'] and k in ('dz', 'da'):
            r[k + '16'] = lx.between16(v, bw64[k], bb32[k], c['io16'])
    return r


def arithmetics(C):
    yield 'fp32 torch', lx.Arith(torch.float32), lx.TREE_N[('rowvec', C)]
    for tree in ('rowvec', 'pair32', 'serial8x16'):
        if (tree, C) in lx.TREE_N:
            for fma in (True, False):
                yield f'{tree}{"" if fma else ", no fma"}', lx.emulation(tree, fma), lx.TREE_N[(tree, C)]


@pytest.mark.parametrize('shape', list(lx.SHAPES))
def test_fp32_evaluations_are_within_every_bound(shape):
    worst = {}
    for kind in lx.KINDS:
        c = lx.rounded_case(kind, **lx.SHAPES[shape])
        for name, ar, n in arithmetics(c['C']):
            r = evaluate(c, ar, n)
            for k, v in r.items():
                assert v <= 1 and (not k.endswith('16') or v == 0), f'{shape} {kind}, {name}: {k} is {v:.3g} x its bound'
                worst[(name, k)] = max(worst.get((name, k), 0.0), v)
    for name in dict.fromkeys(n for n, _ in worst):
        show(f'{shape}, {name}', **{k: v for (n, k), v in worst.items() if n == name})


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------
FAULTS = {       # name: (fault, shape, outputs it must show in)
    'lane_mean': (('lane', 'mean'), 'c128', ('mean', 'y')),
    'lane_s2': (('lane', 's2'), 'c128', ('dz',)),
    'lane_mean_1024': (('lane', 'mean'), 'c1024', ('mean', 'y')),
    'var_over_c_minus_1': ('var_cm1', 'c128', ('rstd', 'y')),
    'eps_missing': ('no_eps', 'c128', ('rstd', 'y')),
    'neighbour_stats': ('neighbour_stats', 'c128', ('dz',)),
    'film_beta_next_utterance': ('film_next', 'c128', ('y',)),
    'row_dropped': (('row_dropped', 4, 100), 'big', ('dw', 'dbias', 'dfilm_gamma', 'dfilm_beta')),
    'block_dropped': (('block_dropped', 0, 1), 'big', ('dw', 'dbias', 'dfilm_gamma', 'dfilm_beta')),
    'wave16_missing': (('wave16',), 'big', ('dw', 'dbias', 'dfilm_gamma', 'dfilm_beta')),
    'pre_mask_row_plus_1': ('pre_mask_row1', 'c128', ('z', 'da')),
    'relu_mask_ge': ('relu_ge', 'c1024', ('dz',)),
    'halo_ignored': ('no_halo', 'c1024', ('y', 'dz')),
}


@pytest.mark.parametrize('name', list(FAULTS))
def test_planted_faults_break_their_bound_by_four(name):
    fault, shape, outputs = FAULTS[name]
    kinds = ('relu',) if name == 'relu_mask_ge' else lx.KINDS
    best = {}
    for kind in kinds:
        c = lx.rounded_case(kind, **lx.SHAPES[shape])
        if (name == 'pre_mask_row_plus_1' and not c['p_pre']) or (name == 'film_beta_next_utterance' and c['film'] is None):
            continue
        r = evaluate(c, lx.emulation('rowvec', True, fault), lx.TREE_N[('rowvec', c['C'])])
        best[kind] = {k: r[k] for k in outputs if k in r}
    show(name, **{f'{kind}.{k}': v for kind, d in best.items() for k, v in d.items()})
    for k in outputs:
        over = [d[k] for d in best.values() if k in d]
        assert over and max(over) >= 4, f'{name}: {k} is at most {max(over):.3g} x its bound'
    for kind, d in best.items():                          # and every kind of input shows it in at least one of them
        assert max(d.values()) >= 4, f'{name}: at most {max(d.values()):.3g} x a bound on the {kind} rows'


def test_skipped_second_grid_stride_pass_leaves_the_sentinel():
    """the forward's wrap case restates a row subset: rows from 32 700 on are in it, so rows a skipped second pass leaves unwritten are seen"""
    rows = lx.wrap_rows()
    total = lx.WRAP['B'] * lx.WRAP['N']
    assert lx.ln_plan(lx.WRAP['B'], lx.WRAP['N'], 128).passes == 2 and int((rows >= lx.ln_plan(lx.WRAP['B'], lx.WRAP['N'], 128).sweep).sum()) == total - 32768 and len(rows) <= 400
    c = lx.rounded_case('randn', C=128, lens=lx.wrap_lens(), with_dy=False, **lx.WRAP)
    z, _ = lx.make_z(c, rows)
    ref, bound = lx.ln_stage(c, rows, z), lx.stage_bounds(c, rows, z, 11)
    got = lx.ln_stage(c, rows, z.float(), lx.emulation('rowvec'))
    assert lx.worst_ratio(got['y'], ref['y'], bound['y'])[0] <= 1
    got['y'][rows >= 32768] = lx.SENTINEL                                   # what the skipped pass leaves
    assert lx.worst_ratio(got['y'], ref['y'], bound['y'])[0] >= 4


@pytest.mark.parametrize('shape', ['c1024_bf16', 'c1024_fp16'])
def test_16_bit_rows_show_an_fp32_level_fault(shape):
    """variance over C - 1 moves rstd by 5e-4 relative, below the 16-bit store's half ulp: against u_h |y| it shows only on the elements
    near zero, but thousands of stored numbers leave the interval between the roundings of the fp32 bound's ends"""
    c = lx.rounded_case('randn', **lx.SHAPES[shape])
    r = evaluate(c, lx.emulation('rowvec', True, 'var_cm1'), 21)
    show(f'{shape}, variance over C - 1', **r)
    assert r['y16'] >= 100
    r = evaluate(c, lx.emulation('rowvec', True, ('lane', 's2')), 21)
    assert r['dz16'] >= 100


def test_fp16_store_bound_covers_the_subnormal_step():
    """the wrap case with fp16 rows holds y values below 2^-14: an fp16 store rounds them by up to 2^-25 whatever their size (the first
    device run showed 2.08 x a bound without that term, on an element of 2.5e-5; this emulation shows the same figure)"""
    c = lx.rounded_case('randn', C=1024, lens=lx.wrap_lens(), io16='fp16', with_dy=False, **lx.WRAP)
    rows = lx.wrap_rows()
    z, _ = lx.make_z(c, rows)
    ref, bound = lx.ln_stage(c, rows, z), lx.stage_bounds(c, rows, z, 21, 'fp16')
    got = lx.ln_stage(c, rows, z.float(), lx.emulation('rowvec'))['y'].to(torch.float16)
    assert lx.worst_ratio(got, ref['y'], bound['y'])[0] <= 1 < lx.worst_ratio(got, ref['y'], bound['y'] - lx.SUB_H['fp16'])[0]


# ---- the exact tier ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(lx.EXACT_BWD))
def test_exact_backward_tier_is_exact_in_fp32(name):
    for p_pre, p_post in lx.EXACT_P:
        c = lx.exact_bwd_case(p_pre=p_pre, p_post=0.0 if name.startswith('ff') else p_post, **lx.EXACT_BWD[name])
        assert lx.representable(torch.nan_to_num(c['z'].float())) and lx.inv_keep(p_pre) in (1.0, 2.0, 4.0)
        ar = lx.Arith()
        ar.trace = {}
        out = lx.ln_backward(c, c['z'], c['mean'], c['rstd'], ar)
        for k, recs in ar.trace.items():
            for value, terms in recs:
                assert lx.representable(value), f'{name}: {k} is not an fp32 number'
                if terms is not None:
                    assert lx.order_free(*terms), f'{name}: a partial sum of {k} may round in some order'
        for k in ('dz', 'da'):
            assert lx.representable(out[k])
        # a fault changes bits
        for fault in ('neighbour_stats', 'pre_mask_row1', ('row_dropped', 0, 0), ('lane', 's2')):
            if fault == 'pre_mask_row1' and not p_pre:
                continue
            bad = lx.ln_backward(c, c['z'], c['mean'], c['rstd'], lx.Arith(torch.float64, 'rowvec' if isinstance(fault, tuple) and fault[0] == 'lane' else None, True, fault))
            assert any(not torch.equal(bad[k], out[k]) for k in out), f'{name}: {fault} changes no bit'


def test_exact_forward_case_has_integer_means():
    for C in (128, 1024):
        c = lx.exact_fwd_case(3, 20, C, [20, 7, 1], p_pre=0.75)
        z, _ = lx.make_z(c, lx.all_rows(c))
        assert lx.representable(z) and bool((z.sum(-1) % C == 0).all()) and float((z * z).sum(-1).max()) < 2 ** 24
        got = lx.ln_stage(c, lx.all_rows(c), z.float(), lx.emulation('rowvec'))
        assert torch.equal(got['mean'].double(), lx.ln_stage(c, lx.all_rows(c), z)['mean'])
