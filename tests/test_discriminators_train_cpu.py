"""CPU checks of the discriminator step: the float64 yardsticks of the GPU tests against the reference fixture, the
power-iteration helper against torch's own spectral norm, argument validation of every new entry point, the Python guards, the price()
entries and the no-scratch rule of csrc/dx_disc_wgrad.hip."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import disc_helpers as dh
from tests import disc_train_torch as dtt
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

PKG = os.path.dirname(os.path.abspath(disc.__file__))


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_float64_autograd_and_the_restated_chain_reproduce_the_reference_gradients(T):
    """disc_torch in float64 with autograd from the parameters gives the fixture's float64 samples and norms (the reference modules
    themselves, norms kept, eval mode) to 1e-9 of each tensor's largest element, and the chain the kernels run, restated layer by
    layer at those float64 maps, gives the autograd gradient of every one of the 154 tensors to 1e-9 too.  sigma is a float64 sum in
    both, so no recorded sigma is needed."""
    z, states = dtt.fixture(T), dh.state_dicts()
    y, y_hat = dh.inputs(T)
    losses, grads, (mo, so) = dtt.autograd_grads(states, y, y_hat)
    assert abs(float(losses['loss_disc_f']) - z['losses64'][0]) <= 1e-12 * z['losses64'][0]
    assert abs(float(losses['loss_disc_s']) - z['losses64'][1]) <= 1e-12 * z['losses64'][1]
    f64 = {d: dtt.folded({k: v.double() for k, v in states[d].items()}, torch.float64) for d in states}
    chain = dtt.chain_grads(states, y, y_hat, f64['mpd'], f64['msd'], dtt.joined_maps(mo), dtt.joined_maps(so))
    n = 0
    for d in ('mpd', 'msd'):
        assert list(grads[d]) == dtt.parameter_keys(states[d]) and set(chain[d]) == set(grads[d])
        for key, g in grads[d].items():
            assert g.shape == states[d][key].shape == chain[d][key].shape, key
            scale = float(g.abs().max())
            want = torch.from_numpy(z[f'{d}/{key}/g64'])
            got = g.flatten()[torch.from_numpy(dh.sample_index(g.numel()))]
            assert float((got - want).abs().max()) <= 1e-9 * scale, (d, key)
            assert abs(float(g.norm()) - z[f'{d}/{key}/norm'][0]) <= 1e-9 * z[f'{d}/{key}/norm'][0], (d, key)
            assert float((chain[d][key] - g).abs().max()) <= 1e-9 * scale, (d, key)
            n += 1
    assert n == 154
    # the predicted decrease of the stored step is what the fixture's docstring says
    sq = sum(float(g.norm()) ** 2 for d in grads for g in grads[d].values())
    assert abs(float(z['eps'].item()) * sq / z['losses64'].sum() - 2e-3) <= 1e-9


@pytest.mark.parametrize('shape', [(128, 32, 41), (1024, 64, 41)])
@pytest.mark.parametrize('n', [1, 3])
def test_power_iterate_is_torchs_train_mode_spectral_norm(shape, n):
    torch.manual_seed(shape[0] + n)
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(shape[1] * 16 if shape[0] == 1024 else shape[1] * 4, shape[0], shape[2],
                                                        groups=16 if shape[0] == 1024 else 4, padding=20))
    assert tuple(conv.weight_orig.shape) == shape
    w, u, v = conv.weight_orig.detach().clone(), conv.weight_u.clone(), conv.weight_v.clone()
    conv.train()
    x = torch.zeros(1, conv.in_channels, 4)
    for _ in range(n):
        conv(x)                                    # one power iteration per train-mode forward
    sigma = disc.power_iterate(w, u, v, n)
    want = torch.dot(conv.weight_u, torch.mv(w.reshape(shape[0], -1), conv.weight_v))
    assert float((u - conv.weight_u).abs().max()) <= 1e-6 and float((v - conv.weight_v).abs().max()) <= 1e-6
    assert abs(float(sigma) - float(want)) <= 1e-6 * float(want)
    assert float((conv.weight.detach() - w / sigma).abs().max()) <= 1e-6 * float((w / sigma).abs().max())


def test_power_iterate_zero_touches_nothing():
    g = torch.Generator().manual_seed(3)
    w, u, v = torch.randn(128, 32, 41, generator=g), torch.randn(128, generator=g), torch.randn(32 * 41, generator=g)
    u0, v0 = u.clone(), v.clone()
    sigma = disc.power_iterate(w, u, v, 0)
    assert torch.equal(u, u0) and torch.equal(v, v0)
    assert torch.equal(sigma, torch.dot(u0, torch.mv(w.reshape(128, -1), v0)))
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match='power_iterations'):
            disc.power_iterate(w, u, v, bad)
    assert torch.equal(u, u0) and torch.equal(v, v0)


def test_wgrad_entry_points_reject_bad_arguments_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    out, s = torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_wgrad_size(6, 70, 128, 512, 1, 5, 3, 2, None, None)
    for bad in ((6, 70, 120, 512, 1, 5, 3, 2), (6, 70, 128, 512, 3, 5, 3, 2), (6, 70, 96, 96, 8, 5, 1, 2), (6, 70, 128, 512, 1, 43, 3, 2),
                (6, 70, 128, 512, 1, 0, 3, 2), (6, 70, 128, 512, 1, 5, 5, 2), (6, 70, 128, 512, 1, 5, 0, 2), (6, 70, 128, 512, 1, 5, 3, 21),
                (6, 3, 128, 512, 1, 5, 3, 0), (0, 70, 128, 512, 1, 5, 3, 2), (6, 70, 128, 64, 16, 41, 2, 20), (6, 70, 128, 48, 1, 5, 3, 2)):
        with pytest.raises(DxError, match='bad shape'):
            L.dx_disc_wgrad_size(*bad, out.data_ptr(), s.data_ptr())
    # 128 -> 512 dense, k 5, stride 3 on 6 rows of 23 positions: 138 k entries in 5 tiles of 32 (the window of a 64-entry tile, 209
    # slots of 64 input channels with the stride-3 halo of up to 4 row segments, would need 89 KB of LDS) -> 5 runs of one tile
    L.dx_disc_wgrad_size(6, 70, 128, 512, 1, 5, 3, 2, out.data_ptr(), s.data_ptr())
    assert int(s) == 5 and int(out) == 5 * (512 * 128 * 5 + 512) * 4
    # the 1024 x 1024 x 5 layer: 21 MB of gradient, so the runs are capped at 3 however long the k axis is
    L.dx_disc_wgrad_size(352, 51, 1024, 1024, 1, 5, 1, 2, out.data_ptr(), s.data_ptr())
    assert int(s) == 3 and int(out) == 3 * (1024 * 1024 * 5 + 1024) * 4
    L.dx_disc_wgrad_size(32, 2048, 128, 256, 16, 41, 2, 20, out.data_ptr(), None)
    assert int(out) == 64 * (256 * 8 * 41 + 256) * 4
    ok = dict(A=4096, sxb=32 * 9 * 3, sxr=32, sxn=96, dZ=8192, szb=128 * 3 * 3, szr=128, szn=384, G=16384, dbias=32768, workspace=65536,
              workspace_bytes=1 << 20, rows=6, rdiv=3, N=9, Cin=32, Cout=128, groups=1, taps=5, stride=3, pad=2, stream=None)

    def wgrad(**kw):
        L.dx_disc_wgrad(*{**ok, **kw}.values())
    for kw, match in ((dict(A=None), 'null'), (dict(dZ=None), 'null'), (dict(G=None), 'null'), (dict(dbias=None), 'null'), (dict(workspace=None), 'null'),
                      (dict(rdiv=0), 'non-positive'), (dict(rows=0), 'bad shape'), (dict(N=0), 'bad shape'), (dict(groups=3), 'bad shape'),
                      (dict(taps=43), 'bad shape'), (dict(stride=5), 'bad shape'), (dict(stride=0), 'bad shape'), (dict(pad=0, N=3), 'bad shape'),
                      (dict(pad=21), 'bad shape'), (dict(Cin=24), 'bad shape'), (dict(Cin=96, Cout=96, groups=8), 'bad shape'),
                      (dict(Cout=48), 'bad shape'), (dict(A=4100), 'aligned'), (dict(szn=130), 'aligned'), (dict(sxr=30), 'aligned'),
                      (dict(workspace_bytes=128 * 32 * 5 * 4), 'smaller than dx_disc_wgrad_size'), (dict(workspace=65540), 'smaller than')):
        with pytest.raises(DxError, match=match):
            wgrad(**kw)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_post_wgrad_size(4, 9, 1024, 3, None)
    for bad in ((0, 9, 1024, 3), (4, 0, 1024, 3), (4, 9, 1022, 3), (4, 9, 1024, 4), (4, 9, 1024, 9)):
        with pytest.raises(DxError, match='bad shape'):
            L.dx_disc_post_wgrad_size(*bad, out.data_ptr())
    L.dx_disc_post_wgrad_size(4, 9, 1024, 3, out.data_ptr())
    assert int(out) == 4 * 8 + 4 * 1024 * 3 * 4                          # 36 score positions in 4 runs
    okp = dict(S=4096, ssb=9, ssr=0, ssn=1, W=4096, A=8192, dZ=16384, sxb=9 * 1024, sxr=0, sxn=1024, gw=4096, s_scale=0.1, dW=32768, db=65536,
               workspace=1 << 20, workspace_bytes=1 << 20, rows=4, half_rows=2, rdiv=1, N=9, C=1024, taps=3, stream=None)

    def post(**kw):
        L.dx_disc_post_wgrad(*{**okp, **kw}.values())
    for kw, match in ((dict(S=None), 'null'), (dict(W=None), 'null'), (dict(A=None), 'null'), (dict(dZ=None), 'null'), (dict(gw=None), 'null'),
                      (dict(dW=None), 'null'), (dict(db=None), 'null'), (dict(workspace=None), 'null'), (dict(C=1022), 'bad shape'),
                      (dict(taps=4), 'bad shape'), (dict(taps=9), 'bad shape'), (dict(rows=0), 'bad shape'), (dict(half_rows=5), 'bad shape'),
                      (dict(half_rows=-1), 'bad shape'), (dict(dZ=16388), 'aligned'), (dict(sxn=1023), 'aligned'), (dict(dZ=8192), 'alias'),
                      (dict(workspace_bytes=1024), 'smaller than dx_disc_post_wgrad_size'), (dict(workspace=(1 << 20) + 4), 'smaller than')):
        with pytest.raises(DxError, match=match):
            post(**kw)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_first_wgrad_size(4, 64, 2, 32, 5, 3, 2, None)
    for bad in ((0, 64, 2, 32, 5, 3, 2), (4, 0, 2, 32, 5, 3, 2), (4, 64, 0, 32, 5, 3, 2), (4, 64, 2, 48, 5, 3, 2), (4, 64, 2, 512, 5, 3, 2),
                (4, 64, 2, 32, 17, 3, 8), (4, 64, 2, 32, 5, 0, 2), (4, 4, 2, 32, 5, 3, 0)):
        with pytest.raises(DxError, match='bad shape'):
            L.dx_disc_first_wgrad_size(*bad, out.data_ptr())
    L.dx_disc_first_wgrad_size(4, 64, 2, 32, 5, 3, 2, out.data_ptr())
    assert int(out) == 8 * 32 * 6 * 4                                    # 4 x 11 x 2 = 88 entries: one run of 8 sub-runs
    okf = dict(x=4096, sxb=64, T=64, dZ=8192, dW=16384, db=32768, workspace=65536, workspace_bytes=1 << 20, R=4, p=2, Cout=32, taps=5, stride=3,
               pad=2, stream=None)

    def first(**kw):
        L.dx_disc_first_wgrad(*{**okf, **kw}.values())
    for kw, match in ((dict(x=None), 'null'), (dict(dZ=None), 'null'), (dict(dW=None), 'null'), (dict(db=None), 'null'), (dict(workspace=None), 'null'),
                      (dict(R=0), 'bad shape'), (dict(sxb=63), 'bad shape'), (dict(Cout=48), 'bad shape'), (dict(taps=17, pad=8), 'bad shape'),
                      (dict(T=3, sxb=3, p=7, pad=4), 'reflect'), (dict(workspace_bytes=1024), 'smaller than dx_disc_first_wgrad_size')):
        with pytest.raises(DxError, match=match):
            first(**kw)


def test_guards_of_the_discriminator_step():
    states = dh.state_dicts()
    both = disc.HiFiGanDiscriminators(states, device='cpu')
    y = torch.zeros(2, 1, 64)
    u0 = both.msd.discriminators[0].convs[1].weight_u.clone()
    for fn in (both.discriminator_loss_grad, both.discriminator_backward):
        with pytest.raises(RuntimeError, match='GPU'):
            fn(y, y)
        with pytest.raises(RuntimeError, match='GPU'):
            fn(y, y.clone().requires_grad_(True), power_iterations=0)     # y_hat is detached: it may require grad
        with pytest.raises(ValueError, match=r'\(B, 1, T\)'):
            fn(y[:, 0], y[:, 0])
        with pytest.raises(ValueError, match='reflect'):
            fn(torch.zeros(1, 1, 4), torch.zeros(1, 1, 4))
        for bad in (-1, 1.5, '1', True):
            with pytest.raises(ValueError, match='power_iterations'):
                fn(y, y, power_iterations=bad)
    # nothing above ran a power iteration
    assert torch.equal(both.msd.discriminators[0].convs[1].weight_u, u0)
    assert all(q.grad is None and not q.requires_grad for m in (both.mpd, both.msd) for q in m.parameters())
    assert sum(1 for m in (both.mpd, both.msd) for _ in m.parameters()) == 154
    both.msd.discriminators[1].convs[2].weight_v.requires_grad_(True)
    with pytest.raises(RuntimeError, match='requires grad'):
        both.discriminator_loss_grad(y, y)
    half = disc.HiFiGanDiscriminators(states, device='cpu', precision='bf16')
    for fn in (half.discriminator_loss_grad, half.discriminator_backward):
        with pytest.raises(RuntimeError, match="precision 'f32' only"):
            fn(y, y)


def test_price_entries_of_the_discriminator_step():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[1]])
    fwd = dict(rows=32, rdiv=1, N=2048, Cin=256, Cout=512, groups=16, taps=41, stride=4, pad=20, bf16=0)
    label, bound, flops, byt = profiling.price('dx_disc_wgrad', fwd, geom)
    nout = (2048 + 40 - 41) // 4 + 1
    assert (label, bound) == ('disc_wgrad_grouped<f32>', 'mfma')
    assert flops == profiling.price('dx_disc_conv', fwd, geom)[2] == 2.0 * 32 * nout * 41 * 16 * 512
    assert byt == 32 * (2048 * 256 + nout * 512) * 4 + 512 * (16 * 41 + 1) * 4
    assert profiling.price('dx_disc_wgrad', dict(fwd, groups=1), geom)[0] == 'disc_wgrad<f32>'
    assert profiling.price('dx_disc_post_wgrad', dict(rows=4, N=9, C=1024), geom)[3] == 4 * 9 * (1 + 3 * 1024) * 4
    assert profiling.price('dx_disc_first_wgrad', dict(R=32, T=8192, p=1, Cout=128, taps=15, stride=1, pad=7), geom)[3] == 32 * (8192 * 128 + 8192) * 4


def test_wgrad_kernels_use_no_scratch():
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not on PATH')
    res = subprocess.run(['hipcc', '-O3', '--offload-arch=gfx950', '-std=c++17', '--cuda-device-only', '-c', '-o', os.devnull,
                          '-Rpass-analysis=kernel-resource-usage', os.path.join(PKG, 'csrc', 'dx_disc_wgrad.hip')],
                         check=True, capture_output=True, text=True)
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)
    assert len(scratch) == 14 and set(scratch) == {'0'}, scratch
