"""CPU checks of the HiFi-GAN discriminators' host side: state-dict layout, weight-norm and spectral-norm folding, the plain-torch
restatement against the reference fixture, argument validation of every new entry point, the guards, and the price() entries."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch.nn.utils import remove_weight_norm, weight_norm

from tests import disc_helpers as dh
from tests import disc_torch
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

PKG = os.path.dirname(os.path.abspath(disc.__file__))


@pytest.fixture(scope='module')
def folded():
    states = dh.state_dicts()
    return {d: disc.fold_state_dict(states[d]) for d in ('mpd', 'msd')}


def _squeeze(folded_d):
    return {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]), b) for k, (w, b) in folded_d.items()}


def test_state_dict_keys_and_shapes_match_reference_manifest():
    man = dh.manifest()
    states = dh.state_dicts()
    for d, cls, count in (('mpd', disc.MultiPeriodDiscriminator, 90), ('msd', disc.MultiScaleDiscriminator, 80)):
        m = cls()
        sd = m.state_dict()
        assert len(sd) == len(man[d]) == count
        assert sorted(sd) == sorted(man[d])
        for k, shape in man[d].items():
            assert list(sd[k].shape) == shape, k
            assert sd[k].dtype == torch.float32
        m.load_state_dict(states[d], strict=True)
        assert all(torch.equal(v, states[d][k]) for k, v in m.state_dict().items())
    sd = disc.MultiPeriodDiscriminator().state_dict()
    assert list(sd['discriminators.0.convs.1.weight_g'].shape) == [128, 1, 1, 1]
    assert list(sd['discriminators.0.convs.1.weight_v'].shape) == [128, 32, 5, 1]
    sd = disc.MultiScaleDiscriminator().state_dict()
    assert sorted(k.split('.')[-1] for k in sd if k.startswith('discriminators.0.convs.2.')) == ['bias', 'weight_orig', 'weight_u', 'weight_v']
    assert sorted(k.split('.')[-1] for k in sd if k.startswith('discriminators.1.convs.2.')) == ['bias', 'weight_g', 'weight_v']


def test_weight_norm_folding_equals_torch_remove_weight_norm():
    states = dh.state_dicts()
    mpd = disc.MultiPeriodDiscriminator()
    mpd.load_state_dict(states['mpd'], strict=True)
    folded = mpd.discriminators[4].folded()
    for name, (w, b) in folded.items():
        v, g = states['mpd'][f'discriminators.4.{name}.weight_v'], states['mpd'][f'discriminators.4.{name}.weight_g']
        m = weight_norm(torch.nn.Conv2d(v.shape[1], v.shape[0], (v.shape[2], 1)))
        m.weight_v.data.copy_(v)
        m.weight_g.data.copy_(g)
        remove_weight_norm(m)
        assert torch.equal(w, m.weight.data[..., 0]), name
        assert torch.equal(w, torch._weight_norm(v, g, 0)[..., 0]), name
        assert torch.equal(b, states['mpd'][f'discriminators.4.{name}.bias'])
    msd = disc.MultiScaleDiscriminator()
    msd.load_state_dict(states['msd'], strict=True)
    for name, (w, _) in msd.discriminators[2].folded().items():
        v, g = states['msd'][f'discriminators.2.{name}.weight_v'], states['msd'][f'discriminators.2.{name}.weight_g']
        assert torch.equal(w, torch._weight_norm(v, g, 0)), name


def test_refresh_weights_and_train_mode():
    msd = disc.MultiScaleDiscriminator()
    d = msd.discriminators[1]
    d._packs = {'stale': None}
    msd.load_state_dict(dh.state_dicts()['msd'], strict=True)         # load_state_dict drops the folded copies
    assert d._packs is None
    d._packs = {'stale': None}
    msd.refresh_weights()
    assert d._packs is None
    before = msd.discriminators[0].folded()
    after = msd.train().discriminators[0].folded()                     # no power iteration: train() changes nothing
    assert all(torch.equal(before[k][0], after[k][0]) for k in before)
    assert not any(p.requires_grad for p in msd.parameters())


def test_spectral_fold_reproduces_the_fixture_scores(folded):
    """eval-mode W = weight_orig / (u . W v) with the fixture's stored u, v -> the reference's scores of the spectral-normed
    sub-discriminator, through the restatement."""
    z = dh.fixture()
    states = dh.state_dicts()
    name = 'discriminators.0.convs.3'
    w, u, v = (states['msd'][f'{name}.{s}'] for s in ('weight_orig', 'weight_u', 'weight_v'))
    sigma = torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
    assert torch.equal(folded['msd'][name][0], w / sigma)
    assert 0.1 < float(sigma) < 10.0                                   # power-iterated: not the tiny sigma of a synthetic u, v
    T = 257
    y, y_hat = dh.inputs(T)
    with torch.no_grad():
        for x, tag in ((y, 'score_r'), (y_hat, 'score_g')):
            score, _ = disc_torch.sub_s(x, disc_torch.split(folded['msd'], 0))
            st = z[f'{T}/msd/0/fmap7/stats']
            assert np.abs(score.numpy().astype(np.float64) - z[f'{T}/msd/0/{tag}']).max() <= 4 * st[4] + 1e-6 * st[6]


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_torch_restatement_matches_reference_fixture(folded, T):
    z = dh.fixture()
    y, y_hat = dh.inputs(T)
    with torch.no_grad():
        outs = {'mpd': disc_torch.mpd(y, y_hat, _squeeze(folded['mpd'])), 'msd': disc_torch.msd(y, y_hat, folded['msd'])}
    for d, i, j in dh.fmap_keys(T):
        drs, dgs, fr, fg = outs[d]
        st = z[f'{T}/{d}/{i}/fmap{j}/stats']
        bound = 4 * st[4] + 1e-6 * st[6]
        r, g = fr[i][j], fg[i][j]
        assert list(r.shape) == list(z[f'{T}/{d}/{i}/fmap{j}/shape']), (d, i, j)
        idx = torch.from_numpy(dh.sample_index(r.numel()))
        for t, tag in ((r, 'r'), (g, 'g')):
            assert np.abs(t.flatten()[idx].numpy().astype(np.float64) - z[f'{T}/{d}/{i}/fmap{j}/{tag}']).max() <= bound, (d, i, j, tag)
        assert abs(float(r.double().mean()) - st[0]) <= bound and abs(float(g.double().abs().mean()) - st[3]) <= bound, (d, i, j)
        if j == len(fr[i]) - 1:
            assert np.abs(drs[i].numpy().astype(np.float64) - z[f'{T}/{d}/{i}/score_r']).max() <= bound
            assert np.abs(dgs[i].numpy().astype(np.float64) - z[f'{T}/{d}/{i}/score_g']).max() <= bound
    for d in ('mpd', 'msd'):
        drs, dgs, fr, fg = outs[d]
        dl, rl, gl = disc_torch.discriminator_loss(drs, dgs)
        gen, gens = disc_torch.generator_loss(dgs)
        fm = disc_torch.feature_loss(fr, fg)
        fms = [torch.mean(torch.abs(a - b)) for x, w in zip(fr, fg) for a, b in zip(x, w)]
        for tag, got in (('disc', [dl] + rl + gl), ('gen', [gen] + gens), ('fm', [fm] + fms)):
            f32, f64 = z[f'{T}/{d}/loss/f32/{tag}'], z[f'{T}/{d}/loss/f64/{tag}']
            got = np.array([float(v) for v in got], dtype=np.float64)
            assert got.shape == f32.shape
            assert (np.abs(got - f64) <= 4 * np.abs(f32 - f64) + 1e-6 * np.abs(f64)).all(), (d, tag)


def test_disc_entry_points_reject_bad_arguments_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    out = torch.zeros(1, dtype=torch.long)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_pack_size(128, 32, 5, 0, None)
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_pack_size(120, 32, 5, 0, out.data_ptr())              # Cout % 16
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_pack_size(128, 12, 5, 0, out.data_ptr())              # 12 channels per group
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_pack_size(128, 32, 43, 1, out.data_ptr())             # taps > 41
    L.dx_disc_pack_size(256, 8, 41, 0, out.data_ptr())                  # K = 328 -> 21 k steps of 16: 16 x 21 x 64 x 4 floats
    assert int(out.item()) == 16 * 21 * 64 * 4 * 4
    L.dx_disc_pack_size(256, 8, 41, 1, out.data_ptr())                  # 11 k steps of 32, bf16
    assert int(out.item()) == 16 * 11 * 64 * 8 * 2
    with pytest.raises(DxError, match='null'):
        L.dx_disc_pack(None, 4096, 128, 32, 5, 0, None)
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_pack(4096, 8192, 128, 0, 5, 0, None)
    ok = dict(X=4096, sxb=32 * 9, sxr=0, sxn=32, Wp=8192, bias=8192, Y=16384, syb=128 * 3, syr=0, syn=128, rows=2, rdiv=1, N=9,
              Cin=32, Cout=128, groups=1, taps=5, stride=3, pad=2, act=1, bf16=0, stream=None)

    def conv(**kw):
        L.dx_disc_conv(*{**ok, **kw}.values())
    for kw, match in ((dict(X=None), 'null'), (dict(Wp=None), 'null'), (dict(bias=None), 'null'), (dict(Y=None), 'null'),
                      (dict(Y=4096), 'alias'), (dict(rows=0), 'non-positive'), (dict(N=0), 'non-positive'), (dict(rdiv=0), 'non-positive'),
                      (dict(groups=3), 'divisible'), (dict(Cin=48, groups=32), 'divisible'), (dict(taps=43), 'unsupported'),
                      (dict(stride=5), 'unsupported'), (dict(stride=0), 'unsupported'), (dict(pad=0, N=3), 'unsupported'),
                      (dict(Cin=24), 'unsupported'), (dict(Cout=96), 'unsupported'), (dict(Cin=64, Cout=64, groups=8), 'unsupported'),
                      (dict(X=4100), 'aligned'), (dict(sxn=33), 'aligned'), (dict(bf16=2), 'bf16'), (dict(act=2), 'act')):
        with pytest.raises(DxError, match=match):
            conv(**kw)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_first(None, 12, 12, 4096, 4096, 8192, 2, 3, 32, 5, 3, 2, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_first(4096, 12, 0, 4096, 4096, 8192, 2, 3, 32, 5, 3, 2, None)
    with pytest.raises(DxError, match='reflect'):
        L.dx_disc_first(4096, 3, 3, 4096, 4096, 8192, 2, 7, 32, 5, 3, 2, None)      # pad 4 >= T 3
    with pytest.raises(DxError, match='null'):
        L.dx_disc_post(4096, 1024, 0, 1024, None, 4096, 8192, 1, 0, 1, 2, 1, 1, 1024, 3, None)
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_post(4096, 1024, 0, 1024, 4096, 4096, 8192, 1, 0, 1, 2, 1, 1, 1022, 3, None)
    with pytest.raises(DxError, match='bad shape'):
        L.dx_disc_post(4096, 1024, 0, 1024, 4096, 4096, 8192, 1, 0, 1, 2, 1, 1, 1024, 4, None)
    with pytest.raises(DxError, match='aligned'):
        L.dx_disc_post(4100, 1024, 0, 1024, 4096, 4096, 8192, 1, 0, 1, 2, 1, 1, 1024, 3, None)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_pool(None, 4096, 2, 7, None)
    with pytest.raises(DxError, match='alias'):
        L.dx_disc_pool(4096, 4096, 2, 7, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_pool(4096, 8192, 2, 0, None)
    with pytest.raises(DxError, match='null'):
        L.dx_disc_losses_workspace(10, 2, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_losses_workspace(0, 2, out.data_ptr())
    L.dx_disc_losses_workspace(16385, 3, out.data_ptr())
    assert int(out.item()) == 3 * 2 * 4
    with pytest.raises(DxError, match='null'):
        L.dx_disc_losses(None, 2, 1, 10, 20, 4096, 8192, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_losses(4096, 0, 1, 10, 20, 4096, 8192, None)
    with pytest.raises(DxError, match='non-positive'):
        L.dx_disc_losses(4096, 2, 0, 10, 20, 4096, 8192, None)
    with pytest.raises(DxError, match='total_count'):
        L.dx_disc_losses(4096, 2, 1, 10, 21, 4096, 8192, None)


def test_guards_no_cpu_path_reflect_and_requires_grad():
    states = dh.state_dicts()
    mpd, msd = disc.MultiPeriodDiscriminator(), disc.MultiScaleDiscriminator()
    mpd.load_state_dict(states['mpd'])
    msd.load_state_dict(states['msd'])
    y = torch.zeros(2, 1, 64)
    for m in (mpd, msd, mpd.discriminators[0], msd.discriminators[0]):
        with pytest.raises(RuntimeError, match='GPU'):
            m(y, y) if m in (mpd, msd) else m(y)
    with pytest.raises(RuntimeError, match='GPU'):
        disc.discriminator_loss([y[:, 0]], [y[:, 0]])
    # torch's reflect pad needs pad < T: period 7 pads 4 samples onto T = 3, period 11 pads 7 onto T = 4; T = 5:
    # 11 - 5 = 6 >= 5 raises too; T = 12 (the fixture's shortest) is fine for every period
    for T in (3, 4, 5):
        with pytest.raises(ValueError, match='reflect'):
            mpd(torch.zeros(1, 1, T), torch.zeros(1, 1, T))
        with pytest.raises(RuntimeError):
            torch.nn.functional.pad(torch.zeros(1, 1, T), (0, 11 - T % 11), 'reflect')
    with pytest.raises(RuntimeError, match='GPU'):
        mpd(torch.zeros(1, 1, 12), torch.zeros(1, 1, 12))
    with pytest.raises(RuntimeError, match='GPU'):
        msd(torch.zeros(1, 1, 3), torch.zeros(1, 1, 3))                 # the MSD has no reflect padding
    with pytest.raises(ValueError, match=r'\(B, 1, T\)'):
        mpd(torch.zeros(2, 64), torch.zeros(2, 64))
    yg = torch.zeros(2, 1, 64, requires_grad=True)
    for m in (mpd, msd):
        with pytest.raises(RuntimeError, match='backward is not built'):
            m(y, yg)
        with torch.no_grad(), pytest.raises(RuntimeError, match='GPU'):
            m(y, yg)
    with pytest.raises(RuntimeError, match='backward is not built'):
        disc.feature_loss([[yg]], [[y]])
    mpd.discriminators[2].convs[1].weight_v.requires_grad_(True)
    with pytest.raises(RuntimeError, match='backward is not built'):
        mpd(y, y)
    with pytest.raises(ValueError, match='precision'):
        disc.MultiPeriodDiscriminator(precision='fp16')
    with pytest.raises(ValueError, match='checkpoint'):
        disc.HiFiGanDiscriminators(None)
    with pytest.raises(TypeError, match='mpd'):
        disc.HiFiGanDiscriminators({'generator': {}}, device='cpu')
    both = disc.HiFiGanDiscriminators(states, device='cpu', precision='bf16')
    assert both.mpd.discriminators[0].precision == 'bf16'
    with pytest.raises(RuntimeError, match='GPU'):
        both.losses(y, y)
    src = open(disc.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+(urllib|huggingface_hub|requests|http)\b', src, flags=re.M)


def test_price_entries():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[1]])
    a = dict(rows=64, rdiv=1, N=2048, Cin=256, Cout=512, groups=16, taps=41, stride=4, pad=20, bf16=0)
    label, bound, flops, byt = profiling.price('dx_disc_conv', a, geom)
    nout = (2048 + 40 - 41) // 4 + 1
    assert (label, bound) == ('disc_conv_grouped<f32>', 'mfma')
    assert flops == 2.0 * 64 * nout * 41 * (256 // 16) * 512
    assert byt == 64 * (2048 * 256 + nout * 512) * 4 + 512 * 16 * 41 * 4
    a = dict(rows=32 * 11, rdiv=11, N=83, Cin=32, Cout=128, groups=1, taps=5, stride=3, pad=2, bf16=1)
    label, _, flops, _ = profiling.price('dx_disc_conv', a, geom)
    assert label == 'disc_conv<bf16>' and flops == 2.0 * 352 * 28 * 5 * 32 * 128
    assert profiling.price('dx_disc_first', dict(B=32, T=8192, p=1, Cout=128, taps=15, stride=1, pad=7), geom)[3] == 32 * (8192 + 8192 * 128) * 4
    assert profiling.price('dx_disc_post', dict(rows=4, N=9, C=1024), geom)[3] == 4 * 9 * 1025 * 4
    assert profiling.price('dx_disc_pool', dict(R=4, T=7), geom)[3] == 4 * (7 + 4) * 4
    assert profiling.price('dx_disc_losses', dict(n=62, n_sets=2, total_count=1000), geom)[3] == 8000 + (6 + 186) * 4


def test_disc_kernels_use_no_scratch():
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not on PATH')
    res = subprocess.run(['hipcc', '-O3', '--offload-arch=gfx950', '-std=c++17', '--cuda-device-only', '-c', '-o', os.devnull,
                          '-Rpass-analysis=kernel-resource-usage', os.path.join(PKG, 'csrc', 'dx_disc.hip')],
                         check=True, capture_output=True, text=True)
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)
    assert len(scratch) >= 13 and set(scratch) == {'0'}, scratch
