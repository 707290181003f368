"""CPU checks of the generator's training path: the float64 oracle against the reference's stored gradients, the training launch list,
``backward_launches`` walked by bookkeeping and interpreted in plain torch against autograd, the host-built data-gradient weights, and
the argument checks of the three new entry points."""
import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_backward_helpers as H
from tests import vocoder_helpers
from ubisoft_laforge_daft_exprt_amd import vocoder as voc
from ubisoft_laforge_daft_exprt_amd import vocoder_train as vt


@pytest.mark.parametrize('name', H.CASES)
def test_oracle_reproduces_the_reference_gradients(name):
    """Ties the test-time oracle to the reference: every stored float64 gradient and the norm of EVERY parameter's gradient to 1e-10."""
    c, got = H.case(name), H.oracle(name)
    assert set(got) == set(c['keys']) and len(c['grads']) >= 2 * len(c['keys']) // 3
    for k, want in c['grads'].items():
        assert got[k].shape == want.shape
        assert ((got[k] - want).norm() / want.norm()).item() <= 1e-10, k
    for k in c['keys']:
        assert abs(got[k].norm().item() - c['norms'][k]) <= 1e-10 * c['norms'][k], k


@pytest.mark.parametrize('name', H.CASES)
def test_training_list_has_conv_and_post_only_and_no_shared_buffer(name):
    config = voc.CONFIGS[name]()
    topo = voc.generator_launches(config, 'f32', training=True)
    assert {ln['kind'] for ln in topo.launches} == {'conv', 'post'}
    slots = [t['slot'] for t in topo.tensors.values()]
    assert len(set(slots)) == len(slots)
    assert sorted(ln['layer'] for ln in topo.launches) == sorted(voc.HiFiGANGenerator(config).layer_names())     # one launch per layer
    # the input of every convolution is a tensor of its own
    assert all(ln['x'] == 'mel' or ln['x'] in topo.tensors for ln in topo.launches)
    with pytest.raises(ValueError, match='f32'):
        voc.generator_launches(config, 'bf16', training=True)
    assert voc.generator_launches(config, 'f32') is voc.generator_launches(config, 'f32', training=False)


@pytest.mark.parametrize('name', H.CASES)
def test_backward_list_walk(name):
    config = voc.CONFIGS[name]()
    topo, plan = voc.generator_launches(config, 'f32', training=True), vt.backward_launches(config)
    final_writer = {}
    for i, ln in enumerate(topo.launches):
        final_writer[ln['y']] = i
    # a saved tensor is complete once its last writer ran; the training list has no launch that writes it afterwards, and none shares its buffer
    saved_ok = set(final_writer) | {'mel'}
    written, wgrads = {'dy'}, []
    for i, s in enumerate(plan.steps):
        assert s['kernel'] in ('post_bwd', 'conv', 'act_bwd', 'wgrad'), i
        assert set(s['saved']) <= saved_ok, (i, s['saved'])
        assert set(s['reads']) <= written, (i, 'reads a gradient buffer no step has written', s['reads'])
        assert all(w in plan.buffers for w in s['writes']), i
        written |= set(s['writes'])
        if s['kernel'] in ('wgrad', 'post_bwd'):
            wgrads.append(s['layer'])
    assert sorted(wgrads) == sorted(ln['layer'] for ln in topo.launches)          # every layer: exactly one weight gradient
    assert not any(s['kernel'] == 'conv' and s['layer'] == 'conv_pre' for s in plan.steps)     # no gradient to the mel
    for s in plan.steps:
        if s['kernel'] == 'conv':                                              # every data gradient is a shape dx_voc_conv accepts
            assert s['cout'] in (16, 32, 64, 128, 256, 512) and s['cin'] % 4 == 0 and s['taps'] % 2 == 1 and s['dil'] * (s['taps'] - 1) <= 72


@pytest.mark.parametrize('name', H.CASES)
def test_backward_list_interpreted_in_float64_equals_autograd(name):
    """The two lists, each kernel replaced by its definition in plain torch (float64, the padded widths the device runs): the folded
    gradients, pushed through weight norm and the padding by autograd, equal the oracle's."""
    c, want = H.case(name), H.oracle(name)
    config = voc.CONFIGS[name]()
    names = voc.HiFiGANGenerator(config).layer_names()
    params = {k: torch.as_tensor(v).double().requires_grad_() for k, v in vocoder_helpers.state_dict(name).items()}
    weights = voc.pad_folded_weights(H.folded(params, names), config)
    with torch.no_grad():
        detached = {k: (w.detach(), b.detach()) for k, (w, b) in weights.items()}
        t = H.run_forward(config, detached, c['mel'].double(), c['lengths'])
        grads = H.run_backward(config, detached, t, c['dy'].double(), c['lengths'])
    outs = [x for n in names for x in weights[n]]
    got = dict(zip(params, torch.autograd.grad(outs, list(params.values()), [x for n in names for x in grads[n]])))
    for k in want:
        assert ((got[k] - want[k]).norm() / want[k].norm()).item() <= 1e-10, k


@pytest.mark.parametrize('k,d', [(3, 1), (7, 3), (11, 5), (5, 6), (7, 12)])
def test_dgrad_weight_equals_conv1d_autograd(k, d):
    g = torch.Generator().manual_seed(k * 100 + d)
    w = torch.randn(6, 4, k, generator=g, dtype=torch.float64)
    x = torch.randn(2, 4, 90, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 6, 90, generator=g, dtype=torch.float64)
    pad = d * (k - 1) // 2
    want, = torch.autograd.grad(F.conv1d(x, w, padding=pad, dilation=d), x, dy)
    got = F.conv1d(dy, vt.dgrad_weight(w), padding=pad, dilation=d)
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize('u', [2, 4, 8])
def test_ups_dgrad_weight_equals_conv_transpose1d_autograd(u):
    g = torch.Generator().manual_seed(u)
    w = torch.randn(6, 4, 2 * u, generator=g, dtype=torch.float64, requires_grad=True)
    x = torch.randn(2, 6, 11, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 4, 11 * u, generator=g, dtype=torch.float64)
    y = F.conv_transpose1d(x, w, stride=u, padding=u // 2)
    want_x, want_w = torch.autograd.grad(y, (x, w), dy)
    dyv = dy.transpose(1, 2).reshape(2, 11, u * 4).transpose(1, 2)                 # the free reshape of the channels-last buffer
    got = F.conv1d(dyv, vt.ups_dgrad_weight(w.detach(), u), padding=1)
    assert (got - want_x).abs().max().item() <= 1e-12
    G, _ = H.wgrad_reference(x.detach().transpose(1, 2), dy.transpose(1, 2), 3, 1, u, 0)     # the weight gradient through the same view
    assert (G - want_w).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        vt.ups_dgrad_weight(w.detach(), u + 1)


def test_new_entry_points_check_their_arguments_before_launching():
    from ubisoft_laforge_daft_exprt_amd._lib import lib, DxError
    L = lib()
    P = 4096                                      # never dereferenced: every call below fails its argument checks
    with pytest.raises(DxError, match='null'):
        L.dx_voc_wgrad(None, 64, 16, 1, P, 64, 16, 0, P, P, P, 1 << 20, P, 1, 1, 4, 16, 16, 3, 1, 1, 1, None)
    with pytest.raises(DxError, match='multiples of 16'):
        L.dx_voc_wgrad(P, 48, 12, 1, P, 64, 16, 0, P, P, P, 1 << 20, P, 1, 1, 4, 12, 16, 3, 1, 1, 1, None)
    with pytest.raises(DxError, match='taps'):
        L.dx_voc_wgrad(P, 64, 16, 1, P, 64, 16, 0, P, P, P, 1 << 20, P, 1, 1, 4, 16, 16, 4, 1, 1, 1, None)
    with pytest.raises(DxError, match='taps'):      # a transposed conv is the three-tap view
        L.dx_voc_wgrad(P, 64, 16, 1, P, 128, 32, 0, P, P, P, 1 << 20, P, 1, 1, 4, 16, 16, 2, 1, 2, 1, None)
    with pytest.raises(DxError, match='act'):
        L.dx_voc_wgrad(P, 64, 16, 1, P, 64, 16, 0, P, P, P, 1 << 20, P, 1, 1, 4, 16, 16, 3, 1, 1, 2, None)
    with pytest.raises(DxError, match='rows that hold'):      # one phase of the view needs rows of up Cout channels
        L.dx_voc_wgrad(P, 64, 16, 1, P, 128, 16, 0, P, P, P, 1 << 20, P, 1, 1, 4, 16, 16, 3, 1, 2, 1, None)
    with pytest.raises(DxError, match='workspace'):
        L.dx_voc_wgrad(P, 64, 16, 1, P, 64, 16, 0, P, P, P, 16, P, 1, 1, 4, 16, 16, 3, 1, 1, 1, None)
    n = torch.zeros(1, dtype=torch.long)
    L.dx_voc_wgrad_size(2, 70, 16, 16, 3, 1, n.data_ptr())
    assert int(n) >= 3 * 16 * 16 * 4 + 16 * 4
    with pytest.raises(DxError, match='bad shape'):
        L.dx_voc_wgrad_size(2, 70, 16, 24, 3, 1, n.data_ptr())
    with pytest.raises(DxError, match='null'):
        L.dx_voc_act_bwd(P, None, None, P, P, 1, 1, 4, 16, 1.0, 0, None)
    with pytest.raises(DxError, match='C %% 4|C % 4'):
        L.dx_voc_act_bwd(P, P, None, P, P, 1, 1, 4, 6, 1.0, 0, None)
    with pytest.raises(DxError, match='acc'):
        L.dx_voc_act_bwd(P, P, None, P, P, 1, 1, 4, 16, 1.0, 2, None)
    with pytest.raises(DxError, match='aligned'):
        L.dx_voc_act_bwd(P, P + 4, None, P, P, 1, 1, 4, 16, 1.0, 0, None)
    with pytest.raises(DxError, match='null'):
        L.dx_voc_post_bwd(P, 64, P, P, None, 4, P + 256, P, P, P, 1 << 20, P, 1, 1, 4, 16, None)
    with pytest.raises(DxError, match='channel count'):
        L.dx_voc_post_bwd(P, 96, P, P, P, 4, P + 256, P, P, P, 1 << 20, P, 1, 1, 4, 24, None)
    with pytest.raises(DxError, match='dX not X'):
        L.dx_voc_post_bwd(P, 64, P, P, P, 4, P, P, P, P, 1 << 20, P, 1, 1, 4, 16, None)
    with pytest.raises(DxError, match='workspace'):
        L.dx_voc_post_bwd(P, 64, P, P, P, 4, P + 256, P, P, P, 8, P, 1, 1, 4, 16, None)
    L.dx_voc_post_bwd_size(2, 70, 32, n.data_ptr())
    assert int(n) == 2 * 225 * 4
