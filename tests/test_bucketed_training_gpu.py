"""Bucketed training (trainer.Trainer(bucket=...), trainer.pad_batch): a micro-batch padded past its longest utterances, with the true maxima
in ``Lengths.exist``, computes what the exact-shape step computes -- forward, the seven loss terms and every parameter gradient -- and one
captured graph serves every batch of a length bucket."""
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _model(precision, hp):
    import ubisoft_laforge_daft_exprt_amd as pkg
    pkg.set_precision(precision)
    try:
        model = pkg.DaftExprt(hp).to(DEV)
        model.load_state_dict(helpers.golden_state_dict(), strict=True)
        crit = pkg.DaftExprtLoss(DEV, hp)
        crit.load_pitch_predictor(helpers.golden_pitch_predictor_state_dict())
    finally:
        pkg.set_precision('f32')
    return model, crit


def _eager_step(model, crit, inputs, targets):
    model.zero_grad(set_to_none=True)
    out = model(inputs)
    total, terms = crit(out, tuple(targets) + (inputs[6], inputs[7]), 1000)
    total.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    return out[3][0].detach(), terms._device_terms.detach().clone(), grads


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_padded_eager_step_equals_exact_step(precision):
    """A C1-sized batch padded into (L + 9, T + 40) with exist = (L, T) against the exact-shape step, dropout off: the mel on valid frames
    (bitwise in f32) and zero beyond, the seven loss terms, all gradients (f32: <= 1e-5 relative; bf16: terms <= 1e-3, cosine >= 0.999)."""
    from ubisoft_laforge_daft_exprt_amd.synth import CONFIGS, synthetic_batch
    from ubisoft_laforge_daft_exprt_amd.trainer import pad_batch
    hp = helpers.golden_hparams()
    model, crit = _model(precision, hp)
    batch = synthetic_batch(**{**CONFIGS['C1'], 'n_speakers': hp.n_speakers})
    inputs, targets = model.parse_batch(DEV, batch)
    L, T = inputs[0].shape[1], inputs[8].shape[2]
    mel0, terms0, g0 = _eager_step(model, crit, inputs, targets)
    pin, ptg = pad_batch(inputs, L + 9, T + 40)
    assert pin[0].shape[1] == L + 9 and pin[8].shape[2] == T + 40
    mel1, terms1, g1 = _eager_step(model, crit, pin, ptg)
    assert float(mel1[:, :, T:].abs().max()) == 0.0
    assert len(g0) == len(g1) == 184
    if precision == 'f32':
        assert torch.equal(mel1[:, :, :T], mel0), _rel(mel1[:, :, :T], mel0)
        for a, b in zip(terms1.tolist(), terms0.tolist()):
            assert abs(a - b) <= 1e-6 * abs(b), (terms1, terms0)
        for k in g0:
            assert _rel(g1[k], g0[k]) <= 1e-5, (k, _rel(g1[k], g0[k]))
    else:
        assert _rel(mel1[:, :, :T], mel0) <= 1e-3
        for a, b in zip(terms1.tolist(), terms0.tolist()):
            assert abs(a - b) <= 1e-3 * abs(b) + 1e-7, (terms1, terms0)
        va = torch.cat([g1[k].double().flatten() for k in g0])
        vb = torch.cat([g0[k].double().flatten() for k in g0])
        assert float(va @ vb / (va.norm() * vb.norm())) >= 0.999


def _bucket_batches(n=6, seed=0):
    """n batches of three distinct exact shapes (L_max, T_max) = (30, 90), (31, 93), (29, 87): all in the (32, 128) bucket of (16, 64)."""
    from ubisoft_laforge_daft_exprt_amd.synth import synthetic_batch
    pattern = [[30, 22, 17, 9], [31, 25, 12, 8], [29, 28, 20, 5]]
    out = []
    for s in range(n):
        lens = pattern[s % 3]
        g = torch.Generator().manual_seed(700 + seed + s)
        dur = torch.randint(2, 4, (len(lens), max(lens)), generator=g)
        dur[0, :lens[0]] = 3                                   # row 0 is the longest on both axes: T_max = 3 L_max
        out.append(synthetic_batch(len(lens), (1, max(lens)), seed=750 + seed + s, n_speakers=3, sym_lengths=lens, durations_int=dur))
    return out


def _train(hp, bucket, use_graphs, cuts, batches):
    from ubisoft_laforge_daft_exprt_amd.trainer import Trainer
    model, crit = _model('bf16', hp)
    t = Trainer(model, crit, hp, use_graphs=use_graphs, cuts=cuts, bucket=bucket)
    losses = [float(t.train_step([b])[0]) for b in batches]
    return t, losses, {k: p.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('cuts', [0, 3])
def test_bucketed_graphs_match_exact_eager_steps(cuts):
    """Trainer(bucket=(16, 64)): six batches of three exact shapes replay ONE graph set, and the losses and the update match the
    exact-shape eager steps within the bars of test_graph_replay_matches_eager_two_phase_step; a batch of another bucket captures one more."""
    from ubisoft_laforge_daft_exprt_amd.synth import synthetic_batch
    hp = helpers.golden_hparams(initial_learning_rate=2e-4, max_learning_rate=2e-3, warmup_steps=10, grad_clip_thresh=5.0)
    batches = _bucket_batches()
    shapes = {(b[0].shape[1], int(b[9].max())) for b in batches}
    assert len(shapes) == 3
    te, le, pe = _train(hp, None, False, 0, batches)
    tg, lg, pg = _train(hp, (16, 64), True, cuts, batches)
    assert len(tg.graphs) == 1
    (g,) = tg.graphs.values()
    assert g.hits == 6 and len(g.graphs) == cuts + 1
    print('exact eager', le, 'bucketed graphs', lg)
    assert abs(le[0] - lg[0]) <= 1e-6 * abs(le[0])
    for a, b in zip(le, lg):
        assert abs(a - b) <= 3e-3 * abs(a), (le, lg)
    p0 = helpers.golden_state_dict()
    dots = na = nb = 0.0
    for k in pe:
        da, db = (pe[k].cpu() - p0[k]).double().flatten(), (pg[k].cpu() - p0[k]).double().flatten()
        dots += float(da @ db); na += float(da @ da); nb += float(db @ db)
    assert dots / (na * nb) ** 0.5 > 0.995
    # a batch of another bucket: L_max = 40 -> Lb = 48
    other = synthetic_batch(3, (1, 40), seed=799, n_speakers=3, sym_lengths=[40, 33, 12])
    tg.train_step([other])
    assert len(tg.graphs) == 2 and g.hits == 6
    with pytest.raises(ValueError):
        tg.resident_batch(other)


@pytest.mark.parametrize('use_graphs', [False, True])
def test_bucketed_step_survives_cloned_length_tensors(use_graphs):
    """The rows that exist travel inside the trainer as ``Lengths.exist``, not as attributes of the caller's tensors: a device-resident batch
    whose length tensors were cloned (which drops anything stuck onto them, the host-lengths hint included) gives, in bucketed mode, the
    loss of the exact-shape eager step at the first-step bar of test_bucketed_graphs_match_exact_eager_steps."""
    hp = helpers.golden_hparams(initial_learning_rate=2e-4, max_learning_rate=2e-3, warmup_steps=10, grad_clip_thresh=5.0)
    batch = _bucket_batches(1)[0]
    dev_batch = [t.to(DEV) if torch.is_tensor(t) else t for t in batch]
    for i in (5, 9):
        dev_batch[i]._dx_host_lengths = batch[i].tolist()
        dev_batch[i] = dev_batch[i].clone()
        assert not hasattr(dev_batch[i], '_dx_host_lengths')
    _, le, _ = _train(hp, None, False, 0, [batch])
    tb, lb, _ = _train(hp, (16, 64), use_graphs, 0, [tuple(dev_batch)])
    print('exact eager', le, 'bucketed, cloned lengths', lb)
    assert len(tb.graphs) == int(use_graphs)
    assert abs(le[0] - lb[0]) <= 1e-6 * abs(le[0]), (le, lb)


def test_forward_and_loss_with_host_lengths_hint_do_not_sync():
    """Length tensors that carry the ``_dx_host_lengths`` hint (as bench.py's resident batch does): forward + loss issue no device -> host
    synchronisation (``torch.cuda.set_sync_debug_mode('error')`` raises on one), after one warm-up call that builds packs and tables."""
    from ubisoft_laforge_daft_exprt_amd.synth import synthetic_batch
    import ubisoft_laforge_daft_exprt_amd as pkg
    hp = pkg.HyperParams(n_speakers=3)                        # dropout on, as in the timed step
    model, crit = _model('bf16', hp)
    batch = synthetic_batch(4, (12, 24), seed=311, n_speakers=3)
    dev_batch = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in batch)
    for i in (5, 9):
        dev_batch[i]._dx_host_lengths = batch[i].tolist()
    inputs, targets = model.parse_batch(DEV, dev_batch)
    assert inputs[5] is dev_batch[5] and inputs[9] is dev_batch[9]

    def run():
        total, terms = crit(model(inputs), tuple(targets) + (inputs[6], inputs[7]), 1000)
        return total, terms
    run()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        total, terms = run()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.isfinite(total).item() and all(v == v for v in terms.values())


def test_bucketed_graph_dropout_draws_new_masks():
    """Dropout on: three replays of one bucketed graph on the same batch give three different finite losses (lr 0: the weights stay put)."""
    import ubisoft_laforge_daft_exprt_amd as pkg
    from ubisoft_laforge_daft_exprt_amd.trainer import Trainer
    hp = pkg.HyperParams(n_speakers=3)
    model, crit = _model('bf16', hp)
    t = Trainer(model, crit, hp.clone(initial_learning_rate=0.0, max_learning_rate=0.0), use_graphs=True, bucket=(16, 64))
    b = _bucket_batches(1)[0]
    losses = [float(t.train_step([b])[0]) for _ in range(3)]
    assert len(t.graphs) == 1
    assert all(torch.isfinite(torch.tensor(losses))) and len(set(losses)) == 3, losses


def test_bucketed_validate_equals_exact_validate():
    """validate() in bucketed mode (one graph for the bucket) == exact-shape validate() on the same batches (one graph per shape)."""
    from ubisoft_laforge_daft_exprt_amd.trainer import Trainer
    hp = helpers.golden_hparams()
    batches = _bucket_batches(3, seed=40)
    res = {}
    for bucket in (None, (16, 64)):
        model, crit = _model('bf16', hp)
        t = Trainer(model, crit, hp, use_graphs=True, bucket=bucket)
        res[bucket] = t.validate(batches)
        assert len(t.val_graphs) == (3 if bucket is None else 1)
    (v0, t0), (v1, t1) = res[None], res[(16, 64)]
    assert abs(v0 - v1) <= 1e-5 * abs(v0), (v0, v1)
    for k in t0:
        assert abs(t0[k] - t1[k]) <= 1e-5 * abs(t0[k]) + 1e-9, (k, t0[k], t1[k])
