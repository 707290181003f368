"""The fine-tuning loop without a GPU: the float64 yardstick against torch's own weight norm and AdamW, the argument checks of the
job-table entry points, the parameter order against the reference's checkpoint manifest, the pricing of the two launches."""
import itertools
import json
import os

import pytest
import torch

from tests import finetune_torch as ft

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _manifest():
    with open(os.path.join(GOLDEN, 'finetune_checkpoint_manifest.json')) as f:
        return json.load(f)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize('hyper', sorted(ft.HYPERS))
@pytest.mark.parametrize('shape', [(7, 123), (1, 224), (33, 20)])
def test_yardstick_equals_torch_weight_norm_and_adamw_in_float64(shape, hyper):
    """wn_adamw_reference, iterated three steps, is torch._weight_norm under autograd + torch.optim.AdamW with a loaded state, to 1e-12
    relative in float64: the yardstick of the GPU tests is torch's, not this package's."""
    h = ft.HYPERS[hyper]
    job = ft.normed_inputs(*shape, seed=3)
    for step0 in (1, 3):
        mo = (job['m_v'], job['s_v'], job['m_g'], job['s_g'])
        theirs = ft.torch_wn_adamw(job['v'], job['g'], job['dW'], mo, step0, h, torch.float64, steps=3)
        v, g = job['v'].double(), job['g'].double()
        for k in range(3):
            ours = ft.wn_adamw_reference(v, g, job['dW'], mo, step0 + k, h)
            v, g, mo = ours['v'], ours['g'], (ours['m_v'], ours['s_v'], ours['m_g'], ours['s_g'])
        for key in ft.NORMED_KEYS:
            assert _rel(ours[key], theirs[key]) <= 1e-12, (key, step0)
        # the update itself, not only the parameter that carries it
        assert _rel(ours['v'] - job['v'].double(), theirs['v'] - job['v'].double()) <= 1e-9
        assert _rel(ours['g'] - job['g'].double(), theirs['g'] - job['g'].double()) <= 1e-9


@pytest.mark.parametrize('hyper', sorted(ft.HYPERS))
def test_plain_yardstick_equals_torch_adamw_in_float64(hyper):
    h = ft.HYPERS[hyper]
    job = ft.plain_inputs(1027, seed=5)
    theirs = ft.torch_adamw(job['p'], job['dW'], job['m'], job['s'], 3, h, torch.float64, steps=3)
    p, m, s = job['p'], job['m'], job['s']
    for k in range(3):
        ours = ft.plain_reference(p, job['dW'], m, s, 3 + k, h)
        p, m, s = ours['p'], ours['m'], ours['s']
    for key in ft.PLAIN_KEYS:
        assert _rel(ours[key], theirs[key]) <= 1e-12, key


def test_torch_float32_is_within_its_own_bar():
    """The bar's form is sound: torch's float32 run against the yardstick has ratio <= 1/4 by construction, and a step that leaves out
    the weight decay misses the exaggerated set's bar by orders of magnitude."""
    h = ft.EXAGGERATED_HYPER
    job = ft.normed_inputs(7, 123, seed=11)
    ref64, ref32 = ft.references(job, 3, h)
    assert max(ft.job_ratios(job, ref32, ref64, ref32).values()) <= 0.25
    mo = (job['m_v'], job['s_v'], job['m_g'], job['s_g'])
    wrong = ft.wn_adamw_reference(job['v'], job['g'], job['dW'], mo, 3, (h[0], h[1], h[2], 0.0))
    assert ft.job_ratios(job, wrong, ref64, ref32)['v'] > 100


def _jobs(rows):
    return torch.tensor(rows, dtype=torch.int64)


def test_job_table_argument_checks_without_a_gpu():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    P = 1 << 20                                               # never dereferenced: the table is laid out on the host
    nbytes, blocks = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    good = [1, 33, 1300, P, P, P, P, P, P, P, P]
    plain = [0, 1, 1027, P, 0, P, P, P, 0, 0, 0]
    jobs = _jobs([good, plain, [1, 32, 5, P, P, P, P, P, P, P, P]])
    L.dx_wn_adamw_table_size(jobs.data_ptr(), 3, nbytes.data_ptr(), blocks.data_ptr())
    assert int(blocks) == 33 + 1 + 8 and int(nbytes) == 3 * 80 + 8 * int(blocks)
    table = torch.zeros(int(nbytes), dtype=torch.uint8)
    L.dx_wn_adamw_table(jobs.data_ptr(), 3, table.data_ptr(), table.numel())
    index = table[3 * 80:].view(torch.int32).reshape(-1, 2)
    assert index[:33].tolist() == [[0, r] for r in range(33)] and index[33].tolist() == [1, 0]
    assert index[34:].tolist() == [[2, 4 * i] for i in range(8)]                          # four short rows to a workgroup
    with pytest.raises(DxError, match='smaller|reports'):
        L.dx_wn_adamw_table(jobs.data_ptr(), 3, table.data_ptr(), table.numel() - 8)

    def bad(row, match, n=1):
        one = _jobs([row])
        with pytest.raises(DxError, match=match):
            L.dx_wn_adamw_table_size(one.data_ptr(), n, nbytes.data_ptr(), blocks.data_ptr())
        with pytest.raises(DxError, match=match):
            L.dx_wn_adamw_table(one.data_ptr(), n, table.data_ptr(), table.numel())

    for i in range(3, 11):                                    # every pointer of a weight-normed job
        bad(good[:i] + [0] + good[i + 1:], 'null pointer')
    for i in (3, 5, 6, 7):                                    # a plain job reads v, dW and its two moments only
        bad(plain[:i] + [0] + plain[i + 1:], 'null pointer')
    bad(good[:6] + [P + 4] + good[7:], 'moments must be 16-byte aligned')
    bad(good[:7] + [P + 8] + good[8:], 'moments must be 16-byte aligned')
    bad(good[:8] + [P + 2] + good[9:], 'moments must be 16-byte aligned')
    bad(good[:3] + [P + 4] + good[4:], 'v, dW and W must be 16-byte aligned')
    bad([1, 4, 6145] + good[3:], 'rows of at most 6144')
    bad([2] + good[1:], 'kind must be')
    bad([1, 0] + good[2:], 'bad shape')
    bad([0, 2] + plain[2:], 'bad shape')
    bad(good, 'no jobs', n=0)
    with pytest.raises(DxError, match='no jobs'):
        L.dx_wn_adamw_table_size(None, 1, nbytes.data_ptr(), blocks.data_ptr())
    with pytest.raises(DxError, match='null output'):
        L.dx_wn_adamw_table_size(jobs.data_ptr(), 3, None, blocks.data_ptr())


def test_launch_argument_checks_without_a_gpu():
    """Every check runs before the launch: none of these reaches the device."""
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    P = 1 << 20
    ok = dict(table=P, njobs=1, blocks=1, lr=2e-4, beta1=0.8, beta2=0.99, eps=1e-8, weight_decay=0.01, step=1, stream=None)
    for kw, match in ((dict(table=None), 'null table'), (dict(table=P + 8), '16-byte aligned'), (dict(njobs=0), 'must be positive'),
                      (dict(blocks=0), 'must be positive'), (dict(step=0), 'step must be at least 1'), (dict(beta1=1.0), r'betas must lie in \[0, 1\)'),
                      (dict(beta2=-0.1), r'betas must lie in \[0, 1\)'), (dict(beta1=float('nan')), 'betas'), (dict(lr=-1.0), 'finite and not negative'),
                      (dict(eps=float('inf')), 'finite and not negative'), (dict(weight_decay=-0.5), 'finite and not negative')):
        with pytest.raises(DxError, match=match):
            L.dx_wn_adamw(*{**ok, **kw}.values())
    for kw, match in ((dict(table=None), 'null table'), (dict(table=P + 4), '16-byte aligned'), (dict(njobs=-1), 'must be positive')):
        a = {**dict(table=P, njobs=1, blocks=1, stream=None), **kw}
        with pytest.raises(DxError, match=match):
            L.dx_wn_fold(*a.values())


def test_parameter_order_is_the_reference_checkpoints():
    """V1: ``HiFiGANGenerator().parameters()`` and ``chain(msd.parameters(), mpd.parameters())`` have the shapes, in order, of the
    reference's ``optim_g`` / ``optim_d`` states, and the state dicts the keys and shapes of its ``g_*`` / ``do_*`` files."""
    import ubisoft_laforge_daft_exprt_amd as pkg
    man = _manifest()
    gen, mpd, msd = pkg.HiFiGANGenerator(), pkg.MultiPeriodDiscriminator(), pkg.MultiScaleDiscriminator()
    assert [list(p.shape) for p in gen.parameters()] == man['optim_g']['shapes']
    assert [list(p.shape) for p in itertools.chain(msd.parameters(), mpd.parameters())] == man['optim_d']['shapes']
    assert len(man['optim_g']['shapes']) == man['optim_g']['param_group']['params'] and len(man['optim_d']['shapes']) == 154
    assert {k: list(v.shape) for k, v in gen.state_dict().items()} == man['g']['generator']
    assert {k: list(v.shape) for k, v in mpd.state_dict().items()} == man['do']['mpd']
    assert {k: list(v.shape) for k, v in msd.state_dict().items()} == man['do']['msd']
    assert man['g']['keys'] == ['generator'] and man['do']['keys'] == ['mpd', 'msd', 'optim_g', 'optim_d', 'steps', 'epoch']
    # the order NormedAdamW derives from the modules is that order
    from ubisoft_laforge_daft_exprt_amd.vocoder_finetune import _layers
    for layers, params in ((_layers('', gen), list(gen.parameters())),
                           (_layers('msd.', msd) + _layers('mpd.', mpd), list(itertools.chain(msd.parameters(), mpd.parameters())))):
        flat = [p for _, m in layers for p in m.parameters(recurse=False)]
        assert len(flat) == len(params) and all(a is b for a, b in zip(flat, params))


def test_fine_tuner_refuses_what_it_does_not_build():
    import ubisoft_laforge_daft_exprt_amd as pkg
    with pytest.raises(ValueError, match='disc_checkpoint is required'):
        pkg.HiFiGanFineTuner({'generator': {}}, None, 'cpu')
    with pytest.raises(ValueError, match="'f32' only"):
        pkg.HiFiGanFineTuner({'generator': {}}, {'mpd': {}, 'msd': {}}, 'cpu', precision='bf16')


def test_learning_rate_decay_is_exponential_lr():
    from ubisoft_laforge_daft_exprt_amd.vocoder_finetune import _decayed
    p = [torch.nn.Parameter(torch.zeros(1))]
    opt = torch.optim.AdamW(p, lr=2e-4, betas=(0.8, 0.99))
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999, last_epoch=-1)
    for k in range(1, 40):
        opt.step()
        sched.step()
        assert abs(_decayed(2e-4, 0.999, k) - opt.param_groups[0]['lr']) <= 1e-15 * opt.param_groups[0]['lr']


def test_the_two_launches_are_priced_from_the_table_log():
    from ubisoft_laforge_daft_exprt_amd import profiling, vocoder_optim
    geom = profiling.Geometry([[4]])
    vocoder_optim.TABLE_LOG[12345] = (1000, 10)
    try:
        assert profiling.price('dx_wn_adamw', dict(table=12345), geom) == ('wn_adamw', 'hbm', None, 1000 * 32 + 10 * 28)
        assert profiling.price('dx_wn_fold', dict(table=12345), geom) == ('wn_fold', 'hbm', None, 8000)
        assert profiling.price('dx_wn_adamw', dict(table=1), geom)[3] is None
    finally:
        del vocoder_optim.TABLE_LOG[12345]
