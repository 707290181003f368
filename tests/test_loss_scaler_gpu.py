"""The dynamic fp16 loss scaler on the device: the decision launch against a host restatement of torch.amp.GradScaler's rules, the
dynamic Adam and the dynamic loss-gradient launches against the static entry points they mirror (bitwise: the scale is a power of
two), and the Trainer in fp16 with captured graphs through overflows, self-recovery, checkpoints, accumulation, buckets and eager mode.

Shapes: the trainer tests' own, ``synthetic_batch(3, (10, 16))`` (16 symbols, 124 frames) and ``synthetic_batch(4, (12, 24))``."""
import io
import math

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ADAM_REL = 2e-6              # the project's Adam bar, used only where the bias-correction words differ from the host's
# The C ABI carries the betas as floats (dx_adam_step does too): these are the values the kernels see, and the host restatement uses them.
# Two backward passes of the same fp32 computation differ by the order in which the weight-gradient kernels' atomics arrive.  The bar for
# "the same computation, summed in another order" is the project's own for fp32 kernels (tests/test_kernels_gpu.py, rel_err < 2e-6, the
# same ratio: largest difference over largest element).  Two STATIC trainers measure 3.0e-8 .. 1.0e-7 over all gradients and 1.3e-7 ..
# 3.3e-7 per parameter tensor on these shapes (fp16, bf16, with and without accumulation), a dynamic against a static one the same.  A
# power-of-two factor lost or applied twice on a path moves every element that path feeds by at least half of that path's share of it.
GRAD_REL = 2e-6
B1, B2 = float(np.float32(0.9)), float(np.float32(0.98))


# -- host restatement of the rules (include/daft_exprt_hip.h, "dynamic loss scaling") -------------------------------------------------
def host_update(st, finite, cfg):
    """One decision: ``st`` = {scale, applied, good_steps, skipped} -> the next one (+ apply, inv_scale_used)."""
    st = dict(st)
    st['inv_scale_used'] = 1.0 / st['scale']
    if not finite:
        st.update(apply=0, skipped=st['skipped'] + 1, good_steps=0, scale=max(st['scale'] * cfg['backoff'], cfg['min']))
    else:
        st.update(apply=1, applied=st['applied'] + 1, good_steps=st['good_steps'] + 1)
        if st['good_steps'] >= cfg['growth_interval']:
            st.update(scale=min(st['scale'] * cfg['growth'], cfg['max']), good_steps=0)
    return st


def public(st):
    return {k: st[k] for k in ('scale', 'applied', 'good_steps', 'skipped')}


def host_bias_corrections(applied):
    return np.float32(1.0 - B1 ** applied), np.float32(math.sqrt(1.0 - B2 ** applied))


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def read_words(words):
    w = words.cpu()
    f = w.view(torch.float32)
    return {'scale': float(f[0]), 'inv_scale_used': float(f[1]), 'apply': int(w[2]), 'applied': int(w[3]), 'good_steps': int(w[4]),
            'skipped': int(w[5]), 'bc1': np.float32(f[6].item()), 'bc2_sqrt': np.float32(f[7].item())}


def make_words(scale, applied=0, good=0, skipped=0):
    host = torch.zeros(8, dtype=torch.int32)
    host.view(torch.float32)[0] = scale
    host[3], host[4], host[5] = applied, good, skipped
    return host.to(DEV)


INF, NAN = float('inf'), float('nan')


# 1 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('start, lo, hi, norms', [
    (4096.0, 1.0, 2.0 ** 24, [1.5, 0.0, INF, 3e38, 7.0, 1e-30, NAN, 2.0, 2.0, 2.0, 2.0]),        # finite x2, inf, finite x3, NaN, finite x4
    (2.0 ** 16, 1.0, 2.0 ** 16, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, INF, 1.0, 1.0, 1.0]),            # starts at loss_scale_max: growth is clamped
    (0.25, 0.25, 2.0 ** 24, [INF, NAN, 1.0, INF, 1.0, 1.0, 1.0, INF]),                           # starts at loss_scale_min: backoff is clamped
])
def test_decision_rules_equal_the_host_restatement(start, lo, hi, norms):
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    cfg = {'growth': 2.0, 'backoff': 0.5, 'growth_interval': 3, 'min': lo, 'max': hi}
    words = make_words(start)
    normsq = torch.zeros(1, dtype=torch.float32, device=DEV)
    st = {'scale': start, 'applied': 0, 'good_steps': 0, 'skipped': 0}
    bc = (np.float32(0.0), np.float32(0.0))
    scales = []
    for nsq in norms:
        normsq.fill_(nsq)
        lib().dx_scaler_update(words.data_ptr(), normsq.data_ptr(), B1, B2, cfg['growth'], cfg['backoff'], cfg['growth_interval'], lo, hi,
                               torch.cuda.current_stream().cuda_stream)
        st = host_update(st, math.isfinite(nsq), cfg)
        got = read_words(words)
        for k in ('scale', 'inv_scale_used', 'apply', 'applied', 'good_steps', 'skipped'):
            assert got[k] == st[k], (k, nsq, got, st)
        if st['apply']:
            want = host_bias_corrections(st['applied'])
            d = (ulps(got['bc1'], want[0]), ulps(got['bc2_sqrt'], want[1]))
            print('applied', st['applied'], 'bias corrections', got['bc1'], got['bc2_sqrt'], 'ulps from the host', d)
            assert max(d) <= 1, (st['applied'], got, want)
            bc = (got['bc1'], got['bc2_sqrt'])
        else:                                                     # a skipped update leaves them as they were
            assert (got['bc1'], got['bc2_sqrt']) == bc
        scales.append(got['scale'])
    assert float(normsq) == norms[-1] or math.isnan(norms[-1])    # the launch only reads the norm
    if start == 4096.0:
        assert scales == [4096.0, 4096.0, 2048.0, 2048.0, 2048.0, 4096.0, 2048.0, 2048.0, 2048.0, 4096.0, 4096.0]
    elif start == hi:
        assert scales[:6] == [hi] * 6 and st['good_steps'] == 0 and scales[6] == hi / 2 and scales[-1] == hi
    else:
        assert scales[:2] == [lo, lo] and st['skipped'] == 4 and max(scales) == 2 * lo


# 2 -------------------------------------------------------------------------------------------------------------------------------------
def _adam_case(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g) * 4096.0 * 0.3             # what a backward on loss * 4096 leaves in the buckets
    m = 0.1 * torch.randn(n, generator=g)
    v = 0.01 * torch.rand(n, generator=g)
    return [t.to(DEV) for t in (p, grad, m, v)]


@pytest.mark.parametrize('max_norm', [INF, 5.0])
def test_dynamic_adam_equals_the_static_one_and_skips_bitwise(max_norm):
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    n, scale, applied0 = 4 * 1283 + 3, 4096.0, 6                  # six blocks of float4s and an odd tail of 3
    hyper = (1e-3, B1, B2, 1e-9, 1e-6)
    stream = torch.cuda.current_stream().cuda_stream
    cfg = (B1, B2, 2.0, 0.5, 1000, 1.0, 2.0 ** 24)

    def sumsq(grad):
        out = torch.zeros(1, dtype=torch.float32, device=DEV)
        lib().dx_sumsq(grad.data_ptr(), n, out.data_ptr(), stream)
        return out

    # static: dx_adam_step with 1 / scale and the step by value
    p0, grad, m0, v0 = _adam_case(n, 5)
    ps, ms, vs = p0.clone(), m0.clone(), v0.clone()
    nsq = sumsq(grad)
    norm_s, other_s = torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    lib().dx_adam_step(ps.data_ptr(), grad.data_ptr(), ms.data_ptr(), vs.data_ptr(), n, *hyper, applied0 + 1, nsq.data_ptr(), max_norm, 1.0 / scale,
                       None, norm_s.data_ptr(), other_s.data_ptr(), stream)
    # dynamic: the decision launch, then dx_adam_step_dyn reading the state
    pd, md, vd = p0.clone(), m0.clone(), v0.clone()
    words = make_words(scale, applied=applied0)
    norm_d, other_d = torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    lib().dx_scaler_update(words.data_ptr(), nsq.data_ptr(), *cfg, stream)
    lib().dx_adam_step_dyn(pd.data_ptr(), grad.data_ptr(), md.data_ptr(), vd.data_ptr(), n, *hyper, nsq.data_ptr(), max_norm, words.data_ptr(),
                           norm_d.data_ptr(), other_d.data_ptr(), stream)
    got = read_words(words)
    assert got['apply'] == 1 and got['applied'] == applied0 + 1 and got['inv_scale_used'] == 1.0 / scale
    want = host_bias_corrections(applied0 + 1)
    same_words = (got['bc1'], got['bc2_sqrt']) == want
    print('bias-correction words equal the host\'s:', same_words, got['bc1'], got['bc2_sqrt'], want)
    assert not torch.equal(ps, p0)                                # the update really moved the parameters
    if max_norm < INF:
        assert float(norm_s) > max_norm                           # the clipping branch is the one that ran
    assert torch.equal(norm_d, norm_s) and float(other_d) == 0.0 == float(other_s)
    for name, a, b in (('p', pd, ps), ('m', md, ms), ('v', vd, vs)):
        if same_words:
            assert torch.equal(a, b), name
        else:
            rel = ((a - b).abs().max() / b.abs().max()).item()
            print(name, 'rel', rel)
            assert rel <= ADAM_REL, (name, rel)
    # one non-finite gradient element: nothing moves, nothing is counted as applied
    p1, m1, v1 = pd.clone(), md.clone(), vd.clone()
    for bad in (INF, NAN):
        grad_bad = grad.clone()
        grad_bad[1234] = bad
        nsq_bad = sumsq(grad_bad)
        assert not math.isfinite(float(nsq_bad))
        before = read_words(words)
        norm_d.zero_()
        other_d.fill_(1.0)
        lib().dx_scaler_update(words.data_ptr(), nsq_bad.data_ptr(), *cfg, stream)
        lib().dx_adam_step_dyn(pd.data_ptr(), grad_bad.data_ptr(), md.data_ptr(), vd.data_ptr(), n, *hyper, nsq_bad.data_ptr(), max_norm,
                               words.data_ptr(), norm_d.data_ptr(), other_d.data_ptr(), stream)
        after = read_words(words)
        assert torch.equal(pd, p1) and torch.equal(md, m1) and torch.equal(vd, v1)
        assert after['apply'] == 0 and after['applied'] == before['applied'] and after['skipped'] == before['skipped'] + 1
        assert after['scale'] == before['scale'] / 2 and after['inv_scale_used'] == 1.0 / before['scale']
        assert not math.isfinite(float(norm_d)) and float(other_d) == 0.0      # norm_out and zero_after behave as in dx_adam_step
    lib().dx_scaler_update(words.data_ptr(), sumsq(grad).data_ptr(), *cfg, stream)      # a finite norm again: apply = 1 ...
    assert read_words(words)['apply'] == 1
    words_skip = make_words(scale, applied=applied0)                                   # ... and a state that says skip, whatever the norm
    lib().dx_adam_step_dyn(pd.data_ptr(), grad.data_ptr(), md.data_ptr(), vd.data_ptr(), n, *hyper, nsq.data_ptr(), max_norm, words_skip.data_ptr(),
                           None, None, stream)
    assert torch.equal(pd, p1) and torch.equal(md, m1) and torch.equal(vd, v1)


def test_skipped_dynamic_adam_leaves_p_m_v_bitwise_untouched():
    """The skip itself, on its own buffers: a non-finite element -> p, m, v bitwise what they were, ``applied`` unmoved."""
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    n = 4 * 1283 + 3
    stream = torch.cuda.current_stream().cuda_stream
    for bad in (INF, NAN):
        p, grad, m, v = _adam_case(n, 6)
        p0, m0, v0 = p.clone(), m.clone(), v.clone()
        grad[12] = bad
        nsq = torch.zeros(1, dtype=torch.float32, device=DEV)
        lib().dx_sumsq(grad.data_ptr(), n, nsq.data_ptr(), stream)
        words = make_words(4096.0, applied=9, good=2, skipped=1)
        lib().dx_scaler_update(words.data_ptr(), nsq.data_ptr(), B1, B2, 2.0, 0.5, 1000, 1.0, 2.0 ** 24, stream)
        lib().dx_adam_step_dyn(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, B1, B2, 1e-9, 1e-6, nsq.data_ptr(), 5.0,
                               words.data_ptr(), None, None, stream)
        got = read_words(words)
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0)
        assert (got['apply'], got['applied'], got['good_steps'], got['skipped'], got['scale']) == (0, 9, 0, 2, 2048.0)


# 3 -------------------------------------------------------------------------------------------------------------------------------------
def _loss_case(precision):
    import ubisoft_laforge_daft_exprt_amd as pkg
    hp = helpers.golden_hparams()                                 # energy weight 0.05 and pitch weight 0.15: both branches run
    assert hp.energy_consistency_weight > 0 and hp.pitch_consistency_weight > 0
    pkg.set_precision(precision)
    try:
        crit = pkg.DaftExprtLoss(DEV, hp)
        crit.load_pitch_predictor(helpers.golden_pitch_predictor_state_dict())
    finally:
        pkg.set_precision('f32')
    g = torch.Generator().manual_seed(11)
    B, M, T, S = 3, 80, 77, 3                                     # two 64-frame tiles, the second one partial
    lens = torch.tensor([77, 60, 33])
    mel_t = (-4 + 2 * torch.randn(B, M, T, generator=g)) * (torch.arange(T)[None, None, :] < lens[:, None, None])
    mel_p = mel_t + 0.3 * torch.randn(B, M, T, generator=g)
    pitch = (torch.rand(B, T, generator=g) > 0.3) * (4.5 + 0.5 * torch.randn(B, T, generator=g))
    tensors = dict(mel_p=mel_p, spk=torch.randn(B, S, generator=g), pm=0.5 * torch.randn(2, 8, generator=g))
    fixed = dict(mel_t=mel_t.to(DEV), lens=lens.to(DEV), ids=torch.tensor([0, 2, 1], device=DEV), pitch=pitch.to(DEV),
                 energy=torch.zeros(B, T, device=DEV))
    return crit, tensors, fixed


def _loss_grads(crit, tensors, fixed, grad_scale):
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in tensors.items()}
    outputs = (leaves['spk'], (leaves['pm'],), None, (leaves['mel_p'], fixed['lens']), None)
    targets = (None, None, None, fixed['mel_t'], fixed['lens'], fixed['ids'], fixed['energy'], fixed['pitch'])
    crit.grad_scale = grad_scale
    try:
        total, terms = crit(outputs, targets, 5000)
        total.backward(gradient=torch.ones((), device=DEV))
    finally:
        crit.grad_scale = None
    return float(total), dict(terms.items()), {k: v.grad.clone() for k, v in leaves.items()}


@pytest.mark.parametrize('precision', ['f32', 'fp16'])
def test_loss_gradients_with_a_device_scale_equal_the_static_path_bitwise(precision):
    """f32: the frozen predictor layer by layer; fp16: its fused chain -- both end in dx_pitch_grad(_dyn).  The host factor 1 / 3 is what
    a trainer with three accumulation steps passes; scale * (1 / 3) on the host is the float the static path is given."""
    crit, tensors, fixed = _loss_case(precision)
    host = 1.0 / 3
    for scale in (1.0, 4096.0, 2.0 ** -3):
        dev_scale = torch.full((1,), scale, dtype=torch.float32, device=DEV)
        tot_s, terms_s, want = _loss_grads(crit, tensors, fixed, scale * host)
        tot_d, terms_d, got = _loss_grads(crit, tensors, fixed, (host, dev_scale))
        # the terms and the total carry no scale (two of the terms are atomic sums over three workgroups: equal up to summation order)
        assert abs(tot_s - tot_d) <= 1e-6 * abs(tot_s) and all(abs(terms_s[k] - terms_d[k]) <= 1e-6 * abs(terms_s[k]) for k in terms_s)
        assert terms_s['energy_consistency_loss'] > 0 and terms_s['pitch_consistency_loss'] > 0
        for k in ('mel_p', 'spk', 'pm'):
            assert torch.isfinite(want[k]).all() and float(want[k].abs().max()) > 0
            assert torch.equal(got[k], want[k]), (precision, scale, k, float((got[k] - want[k]).abs().max()))
        assert float(dev_scale) == scale
    # and the scale really is read on the device at launch time: the same pair object, another value in the tensor
    pair = (host, torch.full((1,), 2.0, dtype=torch.float32, device=DEV))
    a = _loss_grads(crit, tensors, fixed, pair)[2]
    pair[1].fill_(8.0)
    b = _loss_grads(crit, tensors, fixed, pair)[2]
    want = _loss_grads(crit, tensors, fixed, 8.0 * host)[2]
    for k in a:
        assert torch.equal(b[k], want[k]) and not torch.equal(b[k], a[k]), k


# -- trainer ------------------------------------------------------------------------------------------------------------------------------
def _trainer(precision='fp16', trainer_kw=None, **hp_kw):
    import ubisoft_laforge_daft_exprt_amd as pkg
    from ubisoft_laforge_daft_exprt_amd.trainer import Trainer
    hp = helpers.golden_hparams(**hp_kw)
    pkg.set_precision(precision)
    try:
        model = pkg.DaftExprt(hp).to(DEV)
        model.load_state_dict(helpers.golden_state_dict(), strict=True)
        crit = pkg.DaftExprtLoss(DEV, hp)
        crit.load_pitch_predictor(helpers.golden_pitch_predictor_state_dict())
    finally:
        pkg.set_precision('f32')
    return Trainer(model, crit, hp, **(trainer_kw or {}))


def _clean(which=0):
    from ubisoft_laforge_daft_exprt_amd.synth import synthetic_batch
    return synthetic_batch(3, (10, 16), seed=79, n_speakers=3) if which == 0 else synthetic_batch(4, (12, 24), seed=77, n_speakers=3)


def _poisoned(which=0):
    """The same batch with ONE mel target value of 3e38: the L2 gradient 2 (p - 3e38) c overflows fp32 whatever the scale."""
    batch = list(_clean(which))
    batch[8] = batch[8].clone()
    batch[8][0, 0, 0] = 3e38
    return tuple(batch)


SEQ = 'ccpcccc'                                                   # clean, clean, poisoned, clean x4
DYN = dict(dynamic_loss_scale=True, loss_scale=4096.0, loss_scale_growth_interval=3)
DYN_CFG = {'growth': 2.0, 'backoff': 0.5, 'growth_interval': 3, 'min': 1.0, 'max': 2.0 ** 24}


def _run_sequence(t, seq=SEQ):
    """-> per step: scaler_state() as a dict, whether the gradient norm was finite, whether the parameters moved, the loss."""
    out = []
    for c in seq:
        before = t.optimizer.p_all.clone()
        loss, _, norm = t.train_step([_poisoned() if c == 'p' else _clean()])
        out.append({'state': dict(t.scaler_state().items()), 'finite': bool(torch.isfinite(norm)), 'moved': not torch.equal(t.optimizer.p_all, before),
                    'loss': float(loss), 'graphs': len(t.graphs)})
    return out


def _expected_states(seq, start=4096.0, cfg=DYN_CFG):
    st, out = {'scale': start, 'applied': 0, 'good_steps': 0, 'skipped': 0}, []
    for c in seq:
        st = host_update(st, c != 'p', cfg)
        out.append(public(st))
    return out


def _grad_distance(follow, lead):
    """The two trainers' gradient buckets after their own backward passes: (max |a - b| / max |b| over everything, the same ratio taken
    per parameter tensor and its worst value).  The second catches a factor lost on a path that feeds few or small tensors."""
    mine, theirs = follow.reducer.flat_all, lead.reducer.flat_all
    whole = float((mine - theirs).abs().max() / theirs.abs().max())
    worst = 0.0
    for p, (bi, off) in lead.optimizer._slot.items():
        a, b = follow.reducer.flat[bi][off:off + p.numel()], lead.reducer.flat[bi][off:off + p.numel()]
        worst = max(worst, float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)))
    return whole, worst


def _lockstep(lead, follow, micro, steps):
    """Two trainers of one model on the same micro-batches, ``follow``'s optimiser fed the gradient buckets ``lead``'s backward left.

    Why not two independent runs: a training step here is not reproducible run to run.  The weight-gradient kernels accumulate with fp32
    atomics in arrival order, and two STATIC fp16 trainers on this very batch, same weights, differ after five steps by 2.1e-4 .. 2.7e-4
    in the largest parameter difference and in the third loss onwards (41.36961 against 41.36976); bf16 the same (2.3e-4).  Bitwise
    equality between two separate runs is therefore a property of no implementation, the static mode against itself included.  In
    lockstep everything the comparison is about stays: both trainers run their own forward and loss on their own parameters, their
    own backward (its distance from the leader's is returned and asserted by the callers against GRAD_REL) and their own optimiser launch sequence with their own step count, scale
    and bias corrections, for the same number of steps at the same bars -- equal losses, bitwise parameters and moments.
    -> per step (loss of lead, loss of follow, _grad_distance(follow, lead), then per p / m / v: bitwise equal?, relative distance)."""
    inner, dist = follow.optimizer.step, []

    def step(*args, **kw):
        dist.append(_grad_distance(follow, lead))
        follow.reducer.flat_all.copy_(lead.reducer.flat_all)
        return inner(*args, **kw)
    follow.optimizer.step = step
    out = []
    try:
        for _ in range(steps):
            a = float(lead.train_step(micro)[0])
            b = float(follow.train_step(micro)[0])
            out.append((a, b, dist[-1]))
            for name in ('p_all', 'm_all', 'v_all'):
                pair = (getattr(lead.optimizer, name), getattr(follow.optimizer, name))
                out[-1] += (torch.equal(*pair), float((pair[0] - pair[1]).abs().max() / pair[1].abs().max().clamp_min(1e-30)))
    finally:
        follow.optimizer.step = inner
    return out


@pytest.fixture(scope='module')
def graph_run():
    t = _trainer(**DYN)
    return t, _run_sequence(t)


# 4
def test_trainer_fp16_graphs_survive_a_poisoned_batch(graph_run):
    t, steps = graph_run
    want = _expected_states(SEQ)
    assert want[-1] == {'scale': 4096.0, 'applied': 6, 'good_steps': 1, 'skipped': 1} and want[2]['scale'] == 2048.0
    for i, (c, step, st) in enumerate(zip(SEQ, steps, want)):
        print(i, c, step)
        assert step['state'] == st, (i, step, st)
        assert step['finite'] == (c != 'p') and step['moved'] == (c != 'p'), (i, step)
        assert step['graphs'] == 1
    assert math.isfinite(steps[3]['loss']) and steps[3]['moved']  # the step after the poisoned one trains on
    assert t.skipped_steps() == 1 and t.loss_scale == 4096.0 and t.iteration == len(SEQ) + 1      # the iteration counts skipped updates too
    assert next(iter(t.graphs.values())).hits == len(SEQ)
    assert int(t.optimizer.state_dict()['state'][0]['step']) == 6 # the checkpointed Adam step is the number of APPLIED updates


# 5
def test_trainer_recovers_by_itself_from_a_scale_that_is_too_high():
    """From 2^40 the scale halves on every skipped update and the skipped updates are a prefix of the run; the bar is an applied update
    within 28 steps (measured: 27 skipped, the 28th applied at 2^13; the static fp16 tests run this shape at 2^12).  One graph throughout."""
    t = _trainer(dynamic_loss_scale=True, loss_scale=2.0 ** 40, loss_scale_max=2.0 ** 40)
    p0 = t.optimizer.p_all.clone()
    batch, scale, skipped = _clean(), 2.0 ** 40, 0
    for step in range(28):
        _, _, norm = t.train_step([batch])
        st = dict(t.scaler_state().items())
        if st['applied']:
            break
        skipped += 1
        scale /= 2
        assert st == {'scale': scale, 'applied': 0, 'good_steps': 0, 'skipped': skipped} and not torch.isfinite(norm)
        assert torch.equal(t.optimizer.p_all, p0)                 # bitwise fixed during the skipped prefix
    print('first applied update at step', skipped + 1, 'scale', scale)
    assert st == {'scale': scale, 'applied': 1, 'good_steps': 1, 'skipped': skipped}, st
    assert 1 <= skipped < 28 and bool(torch.isfinite(norm)) and not torch.equal(t.optimizer.p_all, p0)
    for extra in range(3):                                        # the skipped updates were a prefix
        t.train_step([batch])
    assert dict(t.scaler_state().items()) == {'scale': scale, 'applied': 4, 'good_steps': 4, 'skipped': skipped}
    assert len(t.graphs) == 1 and next(iter(t.graphs.values())).hits == skipped + 4


# 6
def test_without_overflow_dynamic_and_static_training_are_the_same():
    """Five steps, same weights, same batch, same scale, growth beyond the run: the dynamic trainer (leading) and the static one in
    lockstep (see _lockstep for why).  Equal losses at every step; parameters and both moments bitwise equal at every step when the
    device's bias-correction words are the host's (they are checked), within the Adam bar otherwise."""
    batch = _clean()
    kw = dict(loss_scale=4096.0, loss_scale_growth_interval=10 ** 6)
    td, ts = _trainer(dynamic_loss_scale=True, **kw), _trainer(dynamic_loss_scale=False, **kw)
    assert td.scaler is not None and ts.scaler is None
    words_equal = True
    for step in range(5):
        (ld, ls, gdist, *eq), = _lockstep(td, ts, [batch], 1)
        got = read_words(td.scaler.words)
        words_equal &= (got['bc1'], got['bc2_sqrt']) == host_bias_corrections(step + 1)
        print('step', step + 1, 'loss dynamic', ld, 'static', ls, 'own backward of the static trainer differs from the dynamic one\'s by', gdist,
              '(p, m, v) bitwise / rel:', eq, 'bias-correction words equal the host\'s:', words_equal)
        assert ld == ls
        assert max(gdist) <= GRAD_REL, (step, gdist)            # the dynamic backward is the static one, over all gradients and per tensor
        for name, same, rel in zip('pmv', eq[0::2], eq[1::2]):
            assert same if words_equal else rel <= ADAM_REL, (step, name, rel)
    assert ts.optimizer.step_count == 5 and ts.skipped_steps() == 0
    assert dict(td.scaler_state().items()) == {'scale': 4096.0, 'applied': 5, 'good_steps': 5, 'skipped': 0}


# 7
def test_checkpoint_carries_the_scaler():
    t = _trainer(**DYN)                                           # its own trainer: the extra step below must not reach the shared one
    steps = _run_sequence(t)
    assert [s['state'] for s in steps] == _expected_states(SEQ)
    ck = t.checkpoint()
    assert ck['loss_scaler'] == steps[-1]['state'] and all(type(v) in (int, float) for v in ck['loss_scaler'].values())
    assert set(ck) - {'loss_scaler'} == {'iteration', 'learning_rate', 'best_val_loss', 'state_dict', 'optimizer', 'config_params'}
    buf = io.BytesIO()
    torch.save({k: v for k, v in ck.items() if k != 'config_params'}, buf)
    buf.seek(0)
    t2 = _trainer(**DYN)
    t2.load_checkpoint(torch.load(buf, map_location=DEV, weights_only=True))
    assert dict(t2.scaler_state().items()) == steps[-1]['state'] and t2.iteration == t.iteration
    # an old checkpoint: no entry -> the scale starts from hparams.loss_scale, the bias-correction step from the optimiser state
    t3 = _trainer(dynamic_loss_scale=True, loss_scale=512.0)
    t3.load_checkpoint({k: v for k, v in ck.items() if k != 'loss_scaler'})
    assert dict(t3.scaler_state().items()) == {'scale': 512.0, 'applied': 6, 'good_steps': 0, 'skipped': 0}
    batch = _clean()
    l1 = float(t.train_step([batch])[0])
    l2 = float(t2.train_step([batch])[0])
    s1, s2 = dict(t.scaler_state().items()), dict(t2.scaler_state().items())
    print('next step: loss', l1, l2, 'state', s1, s2)
    assert s1 == s2 == {'scale': 4096.0, 'applied': 7, 'good_steps': 2, 'skipped': 1}
    assert l1 == l2


# 8
def test_accumulation_one_poisoned_micro_batch_skips_the_whole_update():
    clean, bad = _clean(1), _poisoned(1)
    kw = dict(accumulation_steps=2, loss_scale=4096.0, loss_scale_growth_interval=3)
    ts, td = _trainer(dynamic_loss_scale=False, **kw), _trainer(dynamic_loss_scale=True, **kw)
    # Both micro-batches ran on the scale the static trainer uses for both.  The scaler only holds powers of two, so a micro-batch that
    # had seen another scale would enter the accumulated gradient times 2^k, k != 0: with two equal micro-batches every gradient
    # element would be off by a factor (1 + 2^k) / 2, at least 25 %, against GRAD_REL; the lockstep update is then the static one bitwise.
    (ld, ls, gdist, *eq), = _lockstep(td, ts, [clean, clean], 1)
    got = read_words(td.scaler.words)
    print('accumulated step: loss dynamic', ld, 'static', ls, 'gradient distance', gdist, eq)
    assert abs(ls - ld) <= 1e-6 * abs(ls) and max(gdist) <= GRAD_REL, gdist
    for name, same, rel in zip('pmv', eq[0::2], eq[1::2]):
        assert same if (got['bc1'], got['bc2_sqrt']) == host_bias_corrections(1) else rel <= ADAM_REL, (name, rel)
    p1 = td.optimizer.p_all.clone()
    _, _, norm = td.train_step([clean, bad])                      # the SECOND micro-batch is the poisoned one
    assert not torch.isfinite(norm) and torch.equal(td.optimizer.p_all, p1)
    assert dict(td.scaler_state().items()) == {'scale': 2048.0, 'applied': 1, 'good_steps': 0, 'skipped': 1}
    _, _, norm = td.train_step([clean, clean])
    assert torch.isfinite(norm) and not torch.equal(td.optimizer.p_all, p1)
    assert dict(td.scaler_state().items()) == {'scale': 2048.0, 'applied': 2, 'good_steps': 1, 'skipped': 1}
    assert len(td.graphs) == 1


@pytest.mark.parametrize('trainer_kw', [dict(bucket=(16, 64)), dict(use_graphs=False)], ids=['bucketed', 'eager'])
def test_bucketed_and_eager_trainers_follow_the_same_scaler_trajectory(graph_run, trainer_kw):
    t = _trainer(trainer_kw=trainer_kw, **DYN)
    steps = _run_sequence(t)
    assert [s['state'] for s in steps] == [s['state'] for s in graph_run[1]] == _expected_states(SEQ)
    assert [s['moved'] for s in steps] == [c != 'p' for c in SEQ] and [s['finite'] for s in steps] == [c != 'p' for c in SEQ]
    assert len(t.graphs) == (0 if trainer_kw.get('use_graphs') is False else 1)


def test_the_flag_is_inert_outside_fp16():
    """bf16: no scaler exists, the step issues the launches it issued before, and three steps in lockstep with a trainer without the flag
    (see _lockstep: two separate bf16 runs differ by 2.3e-4 after five steps, flag or no flag) leave bitwise the same parameters."""
    from ubisoft_laforge_daft_exprt_amd import _lib
    batch = _clean()
    t0, t1 = _trainer('bf16', dynamic_loss_scale=False), _trainer('bf16', dynamic_loss_scale=True)
    for t in (t0, t1):
        assert t.scaler is None and t.optimizer.scaler is None and t.loss_scale == 1.0 and 'loss_scaler' not in t.checkpoint()
    steps = _lockstep(t0, t1, [batch], 3)
    print(steps)
    for a, b, gdist, *eq in steps:
        assert a == b and all(eq[0::2]) and max(gdist) <= GRAD_REL, (a, b, gdist, eq)
    assert torch.equal(t0.optimizer.p_all, t1.optimizer.p_all)
    for t in (t0, t1):
        assert t.scaler_state() == {'scale': 1.0, 'applied': 3, 'good_steps': 0, 'skipped': 0}
    # the same launches, in the same order, with the flag: none of the dynamic entry points
    names = []
    for t in (t0, t1):
        t.use_graphs = False                                      # issued one by one, so that the recorder sees them
        rec = []
        old = _lib.set_timer(rec)
        try:
            t.train_step([batch])
        finally:
            _lib.set_timer(old)
        names.append([r[0] for r in rec])
    assert names[0] == names[1] and 'dx_adam_step' in names[1] and not any(n.endswith('_dyn') or n == 'dx_scaler_update' for n in names[1])
