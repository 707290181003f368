"""dx_wn_adamw / dx_wn_fold (csrc/dx_vocoder_optim.hip) on the GPU against the float64 yardstick of tests/finetune_torch.py.

The bar, per output tensor class: max|device - float64| <= 4 max|torch float32 - float64| + 4 * 2^-24 * max|scale|; for a parameter the
compared quantity is the UPDATE p' - p taken in float64 from the stored values (finetune_torch.bar_ratio).  Every ratio is printed."""
import functools

import pytest
import torch

from tests import finetune_torch as ft

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FIELDS = {True: ('v', 'g', 'dW', 'm_v', 's_v', 'm_g', 's_g'), False: ('p', 'dW', 'm', 's')}


def _launch(jobs, hyper, step, fold_only=False):
    """jobs: CPU input dicts -> one launch over all of them -> per job the device results, on the CPU.  (+ the stepped device tensors)"""
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    L = lib()
    rows, dev = [], []
    for job in jobs:
        normed = 'v' in job
        d = {k: job[k].to(DEV).contiguous() for k in FIELDS[normed]}
        if normed:
            d['W'] = torch.full_like(d['v'], float('nan'))
            R, n = job['v'].shape
            rows.append([1, R, n] + [d[k].data_ptr() for k in ('v', 'g', 'dW', 'm_v', 's_v', 'm_g', 's_g', 'W')])
        else:
            rows.append([0, 1, job['p'].numel(), d['p'].data_ptr(), 0, d['dW'].data_ptr(), d['m'].data_ptr(), d['s'].data_ptr(), 0, 0, 0])
        dev.append(d)
    table_rows = torch.tensor(rows, dtype=torch.int64)
    nbytes, blocks = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    L.dx_wn_adamw_table_size(table_rows.data_ptr(), len(rows), nbytes.data_ptr(), blocks.data_ptr())
    host = torch.zeros(int(nbytes), dtype=torch.uint8)
    L.dx_wn_adamw_table(table_rows.data_ptr(), len(rows), host.data_ptr(), host.numel())
    table = host.to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    if fold_only:
        L.dx_wn_fold(table.data_ptr(), len(rows), int(blocks), st)
    else:
        lr, (b1, b2), eps, wd = hyper
        L.dx_wn_adamw(table.data_ptr(), len(rows), int(blocks), lr, b1, b2, eps, wd, step, st)
    torch.cuda.synchronize()
    return [{k: t.cpu() for k, t in d.items()} for d in dev]


@functools.lru_cache(maxsize=None)
def _case(hyper, step):
    """The eleven jobs, their references and the single-launch table result, computed once and shared (leave them unchanged)."""
    jobs = ft.all_inputs(seed=100 * step)
    refs = [ft.references(job, step, ft.HYPERS[hyper]) for job in jobs]
    return jobs, refs, _launch(jobs, ft.HYPERS[hyper], step)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if k != 'dW')


CASES = [('reference', 1), ('reference', 3), ('exaggerated', 1), ('exaggerated', 3)]


@pytest.mark.parametrize('hyper,step', CASES)
@pytest.mark.parametrize('j', range(11), ids=[f'{R}x{n}' for R, n in ft.NORMED_SHAPES] + [f'plain{n}' for n in ft.PLAIN_SIZES])
def test_step_within_the_bar_alone_and_in_the_table(j, hyper, step):
    jobs, refs, table = _case(hyper, step)
    alone = _launch([jobs[j]], ft.HYPERS[hyper], step)[0]
    ratios = ft.job_ratios(jobs[j], alone, *refs[j])
    print(f'bar ratios job {j} {hyper} step {step}:', {k: round(r, 3) for k, r in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    assert _same(alone, table[j]), 'the job in the eleven-job table differs bitwise from the job launched alone'
    assert torch.equal(alone['dW'], jobs[j]['dW']), 'the gradient is read only'


def test_two_launches_give_the_same_bits():
    jobs, _, table = _case('exaggerated', 3)
    again = _launch(jobs, ft.EXAGGERATED_HYPER, 3)
    assert all(_same(a, b) for a, b in zip(table, again))


def test_fold_reproduces_the_steps_weight_bitwise_and_is_torchs_fold():
    jobs, _, table = _case('exaggerated', 3)
    normed = [j for j in range(11) if 'v' in jobs[j]]
    stepped = [dict(jobs[j], v=table[j]['v'], g=table[j]['g']) for j in normed]
    folded = _launch(stepped, None, 0, fold_only=True)
    for j, job, got in zip(normed, stepped, folded):
        assert torch.equal(got['W'], table[j]['W']), ft.NORMED_SHAPES[j]
        assert torch.equal(got['v'], job['v']) and torch.equal(got['m_v'], job['m_v'])          # the fold writes W only
        ref64 = torch._weight_norm(job['v'].double(), job['g'].double(), 0)
        ref32 = torch._weight_norm(job['v'], job['g'], 0)
        ratio = ft.bar_ratio('W', got['W'], ref64, ref32)
        print(f'fold bar ratio {ft.NORMED_SHAPES[j]}: {ratio:.3f}')
        assert ratio <= 1.0


def test_fresh_start_moves_every_element_by_the_learning_rate():
    """Zero moments, step 1, the reference's hyper-parameters: AdamW's first update is lr * sign(grad) on top of the decay."""
    h = ft.REFERENCE_HYPER
    lr, _, _, wd = h
    jobs = ft.all_inputs(seed=7, warm=False)
    got = _launch(jobs, h, 1)
    examined = skipped = 0
    for job, out in zip(jobs, got):
        ref64, ref32 = ft.references(job, 1, h)
        for key in (('m_v', 's_v', 'm_g', 's_g') if 'v' in job else ('m', 's')):
            assert ft.bar_ratio(key, out[key], ref64[key], ref32[key]) <= 1.0, key
        if 'v' in job:
            dv, dg = ft.wn_gradients(job['v'], job['g'], job['dW'])
            pairs = [(job['v'], out['v'], dv), (job['g'], out['g'], dg)]
        else:
            pairs = [(job['p'], out['p'], job['dW'].double())]
        for before, after, grad in pairs:
            assert torch.isfinite(after).all()
            move = after.double() - before.double() * (1 - lr * wd)
            big = grad.abs() >= 1e-3 * grad.pow(2).mean().sqrt()
            examined += int(big.sum())
            skipped += int((~big).sum())
            assert bool((torch.sign(move[big]) == -torch.sign(grad[big])).all())
            assert float((move[big].abs() - lr).abs().max()) <= 1e-3 * lr
    share = skipped / (examined + skipped)
    print(f'fresh start: {examined} elements examined, {skipped} not ({100 * share:.3f} %)')
    assert share <= 0.01


def test_normed_adamw_steps_modules_and_speaks_torchs_state_dict():
    """NormedAdamW over two weight-normed layers and a spectral-normed one: one step is the kernel's (bitwise the raw launch), the state
    dict loads into torch.optim.AdamW and back, a state that does not fit raises."""
    from ubisoft_laforge_daft_exprt_amd.discriminators import _SNConv, _WNConv
    from ubisoft_laforge_daft_exprt_amd.vocoder_optim import NormedAdamW
    gen = torch.Generator().manual_seed(1)
    layers = [('a', _WNConv((33, 4, 5, 1))), ('s', _SNConv((6, 3, 7))), ('b', _WNConv((16, 8, 41)))]
    for _, m in layers:
        for k, p in m.named_parameters():
            p.data = 0.5 + torch.rand(p.shape, generator=gen) if k == 'weight_g' else torch.rand(p.shape, generator=gen) - 0.5
        m.to(DEV)
    before = {f'{n}.{k}': p.detach().cpu().clone() for n, m in layers for k, p in m.named_parameters()}
    opt = NormedAdamW(layers, 2.0 ** -4, (0.5, 0.75), 1e-3, 0.25)
    assert opt.keys == ['a.bias', 'a.weight_g', 'a.weight_v', 's.bias', 's.weight_orig', 'b.bias', 'b.weight_g', 'b.weight_v']
    F = opt.folded()
    assert sorted(F) == ['a', 'b'] and F['a'][0].data_ptr() == opt.W['a'].data_ptr() and F['a'][1] is layers[0][1].bias
    for n in ('a', 'b'):                                          # the constructor folded, with dx_wn_fold
        raw = _launch([_fold_job(before[n + '.weight_v'], before[n + '.weight_g'])], None, 0, fold_only=True)[0]['W']
        assert torch.equal(F[n][0].detach().cpu().reshape(raw.shape), raw)
    grads = {'a': (torch.randn(33, 4, 5, generator=gen).to(DEV), torch.randn(33, generator=gen).to(DEV)),
             'b': (torch.randn(16, 8, 41, generator=gen).to(DEV), torch.randn(16, generator=gen).to(DEV)),
             's.bias': torch.randn(6, generator=gen).to(DEV), 's.weight_orig': torch.randn(6, 3, 7, generator=gen).to(DEV)}
    opt.step(grads)
    torch.cuda.synchronize()
    h = (2.0 ** -4, (0.5, 0.75), 1e-3, 0.25)
    for n, m in (layers[0], layers[2]):
        R = m.weight_v.shape[0]
        job = dict(v=before[n + '.weight_v'].reshape(R, -1), g=before[n + '.weight_g'].reshape(R, 1), dW=grads[n][0].cpu().reshape(R, -1),
                   m_v=torch.zeros(R, m.weight_v.numel() // R), s_v=torch.zeros(R, m.weight_v.numel() // R), m_g=torch.zeros(R, 1), s_g=torch.zeros(R, 1))
        raw = _launch([job], h, 1)[0]
        assert torch.equal(m.weight_v.detach().cpu().reshape(R, -1), raw['v']) and torch.equal(m.weight_g.detach().cpu().reshape(R, 1), raw['g'])
        assert torch.equal(opt.W[n].detach().cpu().reshape(R, -1), raw['W'])
    for key in ('s.bias', 's.weight_orig', 'a.bias'):
        n, k = key.split('.')
        m = dict(layers)[n]
        g = grads[key] if key in grads else grads[n][1]
        ref = ft.plain_reference(before[key], g.cpu(), torch.zeros_like(before[key]), torch.zeros_like(before[key]), 1, h)
        assert float((getattr(m, k).detach().cpu().double() - ref['p']).abs().max()) <= 4 * ft.EPS32
    # torch's layout, both ways
    sd = opt.state_dict()
    assert sorted(sd['state']) == list(range(8)) and float(sd['state'][0]['step']) == 1.0
    stand_in = [torch.nn.Parameter(torch.zeros(p.shape)) for p in opt.params]
    theirs = torch.optim.AdamW(stand_in, lr=1.0)
    theirs.load_state_dict({'state': {i: {k: v.cpu() for k, v in s.items()} for i, s in sd['state'].items()}, 'param_groups': sd['param_groups']})
    assert theirs.param_groups[0]['lr'] == 2.0 ** -4 and theirs.param_groups[0]['betas'] == (0.5, 0.75)
    back = theirs.state_dict()
    opt2 = NormedAdamW(layers, 1.0)
    opt2.load_state_dict(back)
    assert opt2.step_count == 1 and opt2.lr == 2.0 ** -4 and opt2.betas == (0.5, 0.75) and opt2.eps == 1e-3 and opt2.weight_decay == 0.25
    assert all(torch.equal(a, b) for a, b in zip(opt2.exp_avg + opt2.exp_avg_sq, opt.exp_avg + opt.exp_avg_sq))
    bad = {'state': dict(back['state']), 'param_groups': [dict(back['param_groups'][0], params=list(range(7)))]}
    with pytest.raises(ValueError, match='7 parameters'):
        opt2.load_state_dict(bad)
    bad = {'state': {**back['state'], 2: dict(back['state'][2], exp_avg=torch.zeros(3))}, 'param_groups': back['param_groups']}
    with pytest.raises(ValueError, match='shape'):
        opt2.load_state_dict(bad)


def _fold_job(v, g):
    R = v.shape[0]
    n = v.numel() // R
    z = torch.zeros(R, n)
    return dict(v=v.reshape(R, n), g=g.reshape(R, 1), dW=z, m_v=z, s_v=z, m_g=torch.zeros(R, 1), s_g=torch.zeros(R, 1))


def test_bad_arguments_return_their_codes():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    t = torch.zeros(64, device=DEV)
    P = t.data_ptr()
    nbytes, blocks = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    for row, match in (([1, 4, 4, P, P, 0, P, P, P, P, P], 'null pointer'), ([1, 4, 4, P, P, P, P + 4, P, P, P, P], 'moments must be 16-byte aligned'),
                       ([1, 1, 6148, P, P, P, P, P, P, P, P], 'rows of at most 6144')):
        jobs = torch.tensor([row], dtype=torch.int64)
        with pytest.raises(DxError, match=match) as e:
            L.dx_wn_adamw_table_size(jobs.data_ptr(), 1, nbytes.data_ptr(), blocks.data_ptr())
        assert 'code 1' in str(e.value)
    st = torch.cuda.current_stream().cuda_stream
    for args, match in (((P, 1, 1, 2e-4, 0.8, 0.99, 1e-8, 0.01, 0, st), 'step must be at least 1'), ((P, 1, 1, 2e-4, 1.0, 0.99, 1e-8, 0.01, 1, st), 'betas'),
                        ((P, 1, 1, 2e-4, 0.8, -0.5, 1e-8, 0.01, 1, st), 'betas'), ((None, 1, 1, 2e-4, 0.8, 0.99, 1e-8, 0.01, 1, st), 'null table')):
        with pytest.raises(DxError, match=match) as e:
            L.dx_wn_adamw(*args)
        assert 'code 1' in str(e.value)
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0
