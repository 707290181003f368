"""``HiFiGANGenerator.forward`` and its backward on the GPU: parameter gradients against the float64 oracle for the three fixture cases,
determinism, the inference path, the training forward, composition with the two merged loss backwards, an optimiser step, the errors."""
import numpy as np
import pytest
import torch

from tests import vocoder_backward_helpers as H
from tests import vocoder_helpers as vh
from ubisoft_laforge_daft_exprt_amd import vocoder as voc

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

MARGIN = 128.0          # over the reference's own fp32 spread of the tensor (see test_gradient_parity_with_the_float64_oracle)
F32_GRADIENT_BAR = 3e-4   # the project's f32 gradient bar: the margin never reaches past it


def _generator(name, **kw):
    gen = voc.HiFiGANGenerator(voc.CONFIGS[name](), **kw).to(DEV)
    gen.load_state_dict(vh.state_dict(name))
    return gen


@pytest.fixture(scope='module')
def runs():
    """Per case: the generator, its training-forward output and the gradients of two independent forward + backward passes."""
    out = {}
    for name in H.CASES:
        c = H.case(name)
        gen = _generator(name)
        mel, dy = c['mel'].to(DEV), c['dy'].to(DEV)
        passes = []
        for _ in range(2):
            gen.zero_grad(set_to_none=True)
            y = gen(mel, lengths=c['lengths'])
            y.backward(dy[:, None, :])
            passes.append({k: p.grad.detach().cpu().clone() for k, p in gen.named_parameters()})
        out[name] = dict(gen=gen, y=y.detach(), passes=passes)
    return out


@pytest.mark.parametrize('name', H.CASES)
def test_gradient_parity_with_the_float64_oracle(runs, name):
    """Every parameter gradient against the test-time float64 oracle, as |g - g64| / |g64| per tensor.  The bar is MARGIN times the
    reference's own fp32 spread for that tensor (the fixture's), and never looser than 3e-4.  The device adds the same products in
    another order (64-position MFMA tiles, then the partial sums), so its error is another draw from the distribution the reference's
    spread is one draw of.  Measured on an MI355X, ratio = device error / reference spread over the tensors of a case:
        V3 (69 tensors):  median 1.15, 90th percentile 1.47, max  2.23 (conv_pre.weight_g);      largest device error 1.3e-6
        V2 (234 tensors): median 1.26, 90th percentile 1.93, max  4.57 (resblocks.11.convs1.0.bias); largest device error 1.7e-6
        V1 (234 tensors): median 1.58, 90th percentile 2.08, max 79.8  (conv_post.bias);             largest device error 5.9e-6
    The tail is made by the few-element tensors, whose reference spread is itself a single draw: conv_post.bias is ONE number, the
    sum over all samples of dy (1 - y^2), which cancels; the reference's fp32 run happened to land 7.3e-8 from float64 there, the
    device (that sum is added in double) 5.9e-6, which is the forward's fp32 error in y seen through the cancellation.  MARGIN = 128
    is the next power of two over 1.5 x that maximum; for a typical tensor (spread 6e-7) the bar is then 8e-5, a quarter of the cap.
    The second assertion holds the bulk where it was measured: the median ratio of a case stays under 4.
    dy is random over the padded samples too, and a leak from there would be an error of order 1, not of order 1e-6."""
    c, want, got = H.case(name), H.oracle(name), runs[name]['passes'][0]
    assert set(got) == set(want)
    ratios = []
    for k in c['keys']:
        assert got[k].shape == want[k].shape and torch.isfinite(got[k]).all(), k
        err = ((got[k].double() - want[k]).norm() / want[k].norm()).item()
        ratios.append(err / c['spreads'][k])
    order = np.argsort(ratios)
    print(f'{name}: device error / reference fp32 spread: median {np.median(ratios):.2f} max {max(ratios):.2f} at {c["keys"][order[-1]]}; '
          f'largest device error {max(r * c["spreads"][k] for r, k in zip(ratios, c["keys"])):.2e}')
    for k, r in zip(c['keys'], ratios):
        err, bar = r * c['spreads'][k], min(MARGIN * c['spreads'][k], F32_GRADIENT_BAR)
        assert err <= bar, (k, err, bar)
    assert np.median(ratios) <= 4.0, np.median(ratios)


@pytest.mark.parametrize('name', H.CASES)
def test_two_backward_passes_give_the_same_bits(runs, name):
    a, b = runs[name]['passes']
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.count_nonzero(a[k]).item() > 0, k


@pytest.mark.parametrize('name', H.CASES)
def test_without_gradients_the_forward_is_infer_batch_bitwise(runs, name):
    c, gen = H.case(name), runs[name]['gen']
    mel = c['mel'].to(DEV)
    want, _ = voc.HiFiGanVocoder(vh.state_dict(name), config=voc.CONFIGS[name](), device=DEV).infer_batch(mel, c['lengths'])
    with torch.no_grad():
        got = gen(mel, lengths=c['lengths'])
    assert got.shape == (mel.shape[0], 1, 256 * mel.shape[2]) and not got.requires_grad
    assert torch.equal(got[:, 0], want)
    full, _ = voc.HiFiGanVocoder(vh.state_dict(name), config=voc.CONFIGS[name](), device=DEV).infer_batch(mel, [mel.shape[2]] * mel.shape[0])
    with torch.no_grad():
        assert torch.equal(gen(mel)[:, 0], full)                               # the reference's signature: every row whole
    frozen = _generator(name).requires_grad_(False)                            # grad mode on, nothing to train: the same path
    assert torch.equal(frozen(mel, lengths=c['lengths'])[:, 0], want)


@pytest.mark.parametrize('name', H.CASES)
def test_training_forward_meets_the_f32_forward_bar(runs, name):
    """The bar tests/test_vocoder_gpu.py states for f32 against the reference's stored fp32 waveform: max <= 1e-5, mean <= 1e-6; and
    the masked samples are 0."""
    g = vh.golden() if name == 'v1' else None
    lengths, mels, wavs = g if g else (lambda v: (v['lengths'], v['mels'], v['wavs']))(vh.variant_golden(name))
    keep = [i for i, n in enumerate(lengths) if n <= 16] or [int(np.argmin(lengths))]     # the short utterances: the test stays quick
    T = max(lengths[i] for i in keep)
    mel = torch.zeros(len(keep), 80, T)
    for row, i in enumerate(keep):
        mel[row, :, :lengths[i]] = torch.from_numpy(np.asarray(mels[i]))
    y = runs[name]['gen'](mel.to(DEV), lengths=[lengths[i] for i in keep])
    assert y.requires_grad
    for row, i in enumerate(keep):
        n = 256 * lengths[i]
        err = np.abs(y[row, 0, :n].detach().cpu().numpy() - wavs[i])
        print(f'{name} training forward vs reference, {lengths[i]} frames: max {err.max():.2e} mean {err.mean():.2e}')
        assert err.max() <= 1e-5 and err.mean() <= 1e-6, (lengths[i], err.max(), err.mean())
        assert torch.count_nonzero(y[row, 0, n:]).item() == 0
    c = H.case(name)                                                             # and the fixture's rows: constant zeros past the length
    for b, n in enumerate(c['lengths']):
        assert torch.count_nonzero(runs[name]['y'][b, 0, 256 * n:]).item() == 0


def test_composition_with_the_mel_and_the_adversarial_backward_is_bitwise():
    """(MelL1Loss + generator_losses).backward() through the generator equals y_g_hat.backward(dy_hat) with dy_hat computed explicitly
    by the two existing paths: the step of finetune_hifigan.py:229-243 end to end."""
    from tests import disc_helpers as dh
    from ubisoft_laforge_daft_exprt_amd import discriminators as disc
    from ubisoft_laforge_daft_exprt_amd import mel as melmod
    T = 2048
    D = disc.HiFiGanDiscriminators(dh.state_dicts(), device=DEV, precision='f32')
    y = dh.inputs(T)[0].to(DEV)
    B = y.shape[0]
    loss_fn = melmod.MelL1Loss(fmax=None, device=DEV)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(B, 80, T // 256, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0).to(DEV)
    target = (torch.randn(B, 80, T // 256, generator=g) - 5.0).to(DEV)
    gen = _generator('v3')

    y_g_hat = gen(x)
    adv = D.generator_losses(y, y_g_hat)
    (loss_fn(y_g_hat[:, 0], [T] * B, target) + adv['loss_gen_s'] + adv['loss_gen_f'] + adv['loss_fm_s'] + adv['loss_fm_f']).backward()
    one = {k: p.grad.clone() for k, p in gen.named_parameters()}

    gen.zero_grad(set_to_none=True)
    y_g_hat2 = gen(x)
    assert torch.equal(y_g_hat2, y_g_hat)
    leaf = y_g_hat2.detach().clone().requires_grad_(True)
    (g_mel,) = torch.autograd.grad(loss_fn(leaf[:, 0], [T] * B, target), leaf)
    g_adv = D.generator_loss_grad(y, y_g_hat2.detach(), (1.0, 1.0, 1.0, 1.0))[1]
    y_g_hat2.backward(g_mel + g_adv)
    for k, p in gen.named_parameters():
        assert torch.equal(p.grad, one[k]), k
        assert torch.count_nonzero(p.grad).item() > 0, k


def test_one_adamw_step_changes_every_parameter_and_leaves_them_finite():
    c = H.case('v2')
    gen = _generator('v2')
    before = {k: p.detach().clone() for k, p in gen.named_parameters()}
    opt = torch.optim.AdamW(gen.parameters(), lr=2e-4, betas=(0.8, 0.99))
    gen(c['mel'].to(DEV), lengths=c['lengths']).backward(c['dy'].to(DEV)[:, None, :])
    opt.step()
    for k, p in gen.named_parameters():
        assert torch.isfinite(p).all(), k
        assert not torch.equal(p.detach(), before[k]), k
    with torch.no_grad():                                                       # the inference path sees the new weights
        new = gen(c['mel'].to(DEV), lengths=c['lengths'])
    old, _ = voc.HiFiGanVocoder(vh.state_dict('v2'), config=voc.v2_config(), device=DEV).infer_batch(c['mel'].to(DEV), c['lengths'])
    assert torch.isfinite(new).all() and not torch.equal(new[:, 0], old)


def test_errors_are_raised():
    c = H.case('v3')
    mel = c['mel'].to(DEV)
    gen = _generator('v3')
    with pytest.raises(RuntimeError, match='no gradient to the mel'):
        gen(mel.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='f32'):
        _generator('v3', precision='bf16')(mel)
    with torch.no_grad():                                                       # bf16 without gradients is the inference path
        assert _generator('v3', precision='bf16')(mel).shape == (2, 1, 256 * mel.shape[2])
    cpu = voc.HiFiGANGenerator(voc.v3_config())
    with pytest.raises(RuntimeError, match='GPU'):
        cpu(c['mel'])
    with pytest.raises(ValueError):
        gen(mel[:, :40])
    y = gen(mel, lengths=c['lengths'])
    y.backward(torch.ones_like(y), retain_graph=True)
    with pytest.raises(RuntimeError, match='second backward'):
        y.backward(torch.ones_like(y))
