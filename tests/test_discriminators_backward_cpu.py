"""CPU checks of the discriminators' backward: the yardsticks of the GPU tests against the reference fixture, argument
validation of every new entry point, the Python guards, the price() entries and the no-scratch rule of csrc/dx_disc_bwd.hip."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import disc_backward_torch as dbt
from tests import disc_helpers as dh
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

PKG = os.path.dirname(os.path.abspath(disc.__file__))
UNIT = (1.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope='module')
def folded():
    mpd, msd = dbt.fixture_folded()
    return {'mpd': mpd, 'msd': msd}


def test_recorded_sigmas_are_this_machines_up_to_the_last_bits():
    """The fixture's spectral-norm sigmas against the ones folded here: the same numbers up to fp32 summation order."""
    z, states = dbt.fixture(), dh.state_dicts()
    names = [k[len('sigma/'):] for k in z if k.startswith('sigma/')]
    assert len(names) == 8
    for name in names:
        w, u, v = (states['msd'][f'{name}.{s}'] for s in ('weight_orig', 'weight_u', 'weight_v'))
        sigma = float(torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v)))
        assert abs(sigma - float(z['sigma/' + name])) <= 16 * 2.0 ** -24 * abs(sigma), name


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_float64_autograd_and_the_linearised_helper_reproduce_the_reference_gradient(folded, T):
    """disc_torch in float64 with autograd gives the fixture's float64 gradient (the reference modules themselves), and the surrogate
    linearised at the float64 maps gives it too: relative max|d| <= 1e-10 and 1e-9.  The weights are the fixture's to the bit
    (disc_backward_torch.fixture_folded): with the spectral-norm sigmas folded on another CPU, whose fp32 sums differ in the last bit,
    the same comparison gave 4.4e-11 at T = 257 and 1.3e-10 at T = 2048."""
    z = dbt.fixture()
    y, y_hat = dh.inputs(T)
    want = torch.from_numpy(z[f'{T}/grad64'])
    got, (mo, so) = dbt.autograd_grad(y, y_hat, folded['mpd'], folded['msd'], UNIT)
    scale = float(want.abs().max())
    assert got.shape == want.shape == y_hat.shape
    assert float((got - want).abs().max()) <= 1e-10 * scale
    detach = lambda out: ([[t.detach() for t in fm] for fm in out[2]], [[t.detach() for t in fm] for fm in out[3]])
    lin = dbt.linearised_grad(y_hat, folded['mpd'], folded['msd'], detach(mo), detach(so), UNIT)
    assert float((lin - want).abs().max()) <= 1e-9 * scale
    # the stored float32 gradient is the reference's own fp32 autograd: its distance from float64 is what the GPU bars scale with
    g32 = torch.from_numpy(z[f'{T}/grad32']).double()
    assert 0 < float((g32 - want).norm() / want.norm()) < 1e-4


def test_backward_entry_points_reject_bad_arguments_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    out = torch.zeros(1, dtype=torch.long)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_dgrad_pack_size(128, 512, 1, 5, 3, 0, None)
    for bad in ((120, 512, 1, 5, 3, 0), (128, 512, 3, 5, 3, 0), (96, 96, 8, 5, 1, 0), (128, 512, 1, 43, 3, 0), (128, 512, 1, 5, 5, 0),
                (128, 512, 1, 2, 3, 0), (128, 512, 1, 5, 3, 2), (128, 64, 16, 41, 2, 0)):
        with pytest.raises(DxError, match='bad shape'):
            L.dx_disc_dgrad_pack_size(*bad, out.data_ptr())
    # 128 -> 512 dense, k 5, stride 3: phases of 2, 2 and 1 taps, 64 co per chunk, 8 chunks, 8 column blocks
    L.dx_disc_dgrad_pack_size(128, 512, 1, 5, 3, 0, out.data_ptr())
    assert int(out.item()) == (8 + 8 + 4) * 8 * 8 * 64 * 4 * 4
    L.dx_disc_dgrad_pack_size(128, 512, 1, 5, 3, 1, out.data_ptr())
    assert int(out.item()) == (4 + 4 + 2) * 8 * 8 * 64 * 8 * 2
    # 128 -> 256 in 16 groups, k 41, stride 2: 8 input channels per group -> 32 co per column block (two groups, block-diagonal)
    L.dx_disc_dgrad_pack_size(128, 256, 16, 41, 2, 0, out.data_ptr())
    assert int(out.item()) == (21 * 2 + 20 * 2) * 8 * 64 * 4 * 4
    with pytest.raises(DxError, match='null'):
        L.dx_disc_dgrad_pack(None, 4096, 128, 512, 1, 5, 3, 0, None)
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_dgrad_pack(4096, 8192, 128, 512, 0, 5, 3, 0, None)
    ok = dict(dZ=4096, szb=128 * 3, szr=0, szn=128, Wp=8192, dX=16384, R=32768, G=65536, sxb=32 * 9, sxr=0, sxn=32, gw_fm=4096, fm_scale=0.5,
              rows=2, rdiv=1, N=9, Cin=32, Cout=128, groups=1, taps=5, stride=3, pad=2, epilogue=1, bf16=0, stream=None)

    def dgrad(**kw):
        L.dx_disc_conv_dgrad(*{**ok, **kw}.values())
    for kw, match in ((dict(dZ=None), 'null'), (dict(Wp=None), 'null'), (dict(dX=None), 'null'), (dict(R=None), 'null'), (dict(G=None), 'null'),
                      (dict(gw_fm=None), 'null'), (dict(dX=4096), 'alias'), (dict(rows=0), 'non-positive'), (dict(N=0), 'non-positive'),
                      (dict(rdiv=0), 'non-positive'), (dict(groups=3), 'divisible'), (dict(taps=43), 'unsupported'), (dict(stride=5), 'unsupported'),
                      (dict(stride=0), 'unsupported'), (dict(pad=0, N=3), 'unsupported'), (dict(pad=21), 'unsupported'), (dict(Cin=24), 'unsupported'),
                      (dict(Cin=96, Cout=96, groups=8), 'unsupported'), (dict(dZ=4100), 'aligned'), (dict(szn=130), 'aligned'),
                      (dict(bf16=2), 'bf16'), (dict(epilogue=2), 'epilogue')):
        with pytest.raises(DxError, match=match):
            dgrad(**kw)
    okp = dict(Sr=4096, Sg=8192, ssb=9, ssr=0, ssn=1, W=4096, dZ=16384, R=32768, G=65536, sxb=9 * 1024, sxr=0, sxn=1024, gw_gen=4096, gw_fm=4100,
               s_scale=0.1, fm_scale=0.1, rows=2, rdiv=1, N=9, C=1024, taps=3, epilogue=1, stream=None)

    def post(**kw):
        L.dx_disc_post_bwd(*{**okp, **kw}.values())
    for kw, match in ((dict(Sr=None), 'null'), (dict(Sg=None), 'null'), (dict(W=None), 'null'), (dict(dZ=None), 'null'), (dict(R=None), 'null'),
                      (dict(gw_gen=None), 'null'), (dict(gw_fm=None), 'null'), (dict(C=1022), 'bad shape'), (dict(taps=4), 'bad shape'),
                      (dict(rows=0), 'bad shape'), (dict(dZ=16388), 'aligned'), (dict(sxn=1023), 'aligned'), (dict(epilogue=3), 'epilogue')):
        with pytest.raises(DxError, match=match):
            post(**kw)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_first_bwd(None, 4096, 8192, 12, 12, 2, 3, 32, 5, 3, 2, 0, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_first_bwd(4096, 4096, 8192, 12, 0, 2, 3, 32, 5, 3, 2, 0, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_first_bwd(4096, 4096, 8192, 11, 12, 2, 3, 32, 5, 3, 2, 0, None)      # row stride shorter than the row
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_first_bwd(4096, 4096, 8192, 12, 12, 2, 3, 30, 5, 3, 2, 0, None)      # Cout % 4
    with pytest.raises(DxError, match='reflect'):
        L.dx_disc_first_bwd(4096, 4096, 8192, 3, 3, 2, 7, 32, 5, 3, 2, 0, None)
    with pytest.raises(DxError, match='accumulate'):
        L.dx_disc_first_bwd(4096, 4096, 8192, 12, 12, 2, 3, 32, 5, 3, 2, 2, None)
    with pytest.raises(DxError, match='aligned'):
        L.dx_disc_first_bwd(4100, 4096, 8192, 12, 12, 2, 3, 32, 5, 3, 2, 0, None)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_pool_bwd(None, 4096, 2, 7, 0, None)
    with pytest.raises(DxError, match='alias'):
        L.dx_disc_pool_bwd(4096, 4096, 2, 7, 0, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_pool_bwd(4096, 8192, 2, 0, 0, None)
    with pytest.raises(DxError, match='accumulate'):
        L.dx_disc_pool_bwd(4096, 8192, 2, 7, 3, None)


def test_guards_of_the_differentiable_entry_points():
    states = dh.state_dicts()
    both = disc.HiFiGanDiscriminators(states, device='cpu')
    y = torch.zeros(2, 1, 64)
    yg = torch.zeros(2, 1, 64, requires_grad=True)
    for fn in (both.generator_losses, both.generator_loss_grad):
        with pytest.raises(RuntimeError, match='GPU'):
            fn(y, y)
        with pytest.raises(RuntimeError, match='GPU'):
            fn(y, yg)
        with pytest.raises(ValueError, match=r'\(B, 1, T\)'):
            fn(y[:, 0], y[:, 0])
        with pytest.raises(ValueError, match='reflect'):
            fn(torch.zeros(1, 1, 4), torch.zeros(1, 1, 4))
    # the forward-only entry points keep their guard
    with pytest.raises(RuntimeError, match='backward is not built'):
        both.losses(y, yg)
    with pytest.raises(RuntimeError, match='backward is not built'):
        both.mpd(y, yg)
    # y and the parameters are constants
    for fn in (both.generator_losses, both.generator_loss_grad):
        with pytest.raises(RuntimeError, match='y must not require grad'):
            fn(yg, y)
    both.msd.discriminators[1].convs[2].weight_v.requires_grad_(True)
    for fn in (both.generator_losses, both.generator_loss_grad):
        with pytest.raises(RuntimeError, match='parameters are constants'):
            fn(y, yg)
    assert disc.GEN_LOSS_NAMES == ('loss_gen_f', 'loss_fm_f', 'loss_gen_s', 'loss_fm_s')


def test_a_backward_after_a_later_pass_raises():
    """The pass counter of the per-(B, T) plan: a state whose maps were overwritten is refused before anything is launched."""
    both = disc.HiFiGanDiscriminators(dh.state_dicts(), device='cpu')
    plan = disc._Plan()
    for _ in range(3):
        plan.begin()
    with pytest.raises(RuntimeError, match='overwritten by a later pass'):
        both._backward(plan, 2, torch.zeros(4))


def test_price_entries_of_the_backward():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[1]])
    fwd = dict(rows=32, rdiv=1, N=2048, Cin=256, Cout=512, groups=16, taps=41, stride=4, pad=20, bf16=0)
    label, bound, flops, byt = profiling.price('dx_disc_conv_dgrad', dict(fwd, epilogue=1), geom)
    nout = (2048 + 40 - 41) // 4 + 1
    assert (label, bound) == ('disc_dgrad_grouped<f32>', 'mfma')
    assert flops == profiling.price('dx_disc_conv', fwd, geom)[2] == 2.0 * 32 * nout * 41 * 16 * 512
    assert byt == 32 * (nout * 512 + 3 * 2048 * 256) * 4 + 512 * 16 * 41 * 4
    fwd = dict(rows=16 * 11, rdiv=11, N=83, Cin=32, Cout=128, groups=1, taps=5, stride=3, pad=2, bf16=1)
    label, _, flops, byt = profiling.price('dx_disc_conv_dgrad', dict(fwd, epilogue=0), geom)
    assert label == 'disc_dgrad<bf16>' and flops == profiling.price('dx_disc_conv', fwd, geom)[2] == 2.0 * 176 * 28 * 5 * 32 * 128
    assert byt == 176 * (28 * 128 + 83 * 32) * 4 + 128 * 32 * 5 * 2
    assert profiling.price('dx_disc_post_bwd', dict(rows=4, N=9, C=1024, epilogue=1), geom)[3] == 4 * 9 * (2 + 3 * 1024) * 4
    assert profiling.price('dx_disc_first_bwd', dict(B=16, T=8192, p=1, Cout=128, taps=15, stride=1, pad=7, accumulate=1), geom)[3] == \
        16 * (8192 * 128 + 2 * 8192) * 4
    assert profiling.price('dx_disc_pool_bwd', dict(R=4, T=7, accumulate=0), geom)[3] == 4 * (4 + 7) * 4
    assert profiling.price('dx_disc_dgrad_pack', dict(Cin=128, Cout=256, groups=16, taps=41, bf16=1), geom)[3] == 256 * 8 * 41 * 6


def test_backward_kernels_use_no_scratch():
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not on PATH')
    res = subprocess.run(['hipcc', '-O3', '--offload-arch=gfx950', '-std=c++17', '--cuda-device-only', '-c', '-o', os.devnull,
                          '-Rpass-analysis=kernel-resource-usage', os.path.join(PKG, 'csrc', 'dx_disc_bwd.hip')],
                         check=True, capture_output=True, text=True)
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)
    assert len(scratch) == 11 and set(scratch) == {'0'}, scratch
