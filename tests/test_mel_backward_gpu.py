"""The mel front end's waveform gradient on the GPU (csrc/dx_mel.hip, dx_mel_bwd): parity with the fp64 gradients of
tests/golden/mel_backward.npz under bars set by the reference's own fp32 spread, the clamp, valid lengths and bitwise batch rows,
the autograd surface, the reference-signature drop-in, MelL1Loss, and graph capture of forward + loss + backward."""
import numpy as np
import pytest
import torch

from tests import mel_grad_helpers as gh
from tests import mel_helpers as mh
from ubisoft_laforge_daft_exprt_amd import mel

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return gh.golden()


@pytest.fixture(scope='module')
def frontends():
    return {v: mel.MelSpectrogram(fmax=fmax, device=DEV) for v, fmax in mh.FMAX.items()}


def _dwav(fe, wav, lengths, g):
    """Waveform gradient of sum(g . mels) through the autograd surface."""
    w = wav.detach().clone().requires_grad_(True)
    mels, _, _ = fe(w, lengths)
    mels.backward(g)
    return w.grad


def _within(what, name, v, got, f64, spread):
    dd = np.abs(got.astype(np.float64) - f64)
    top = np.abs(f64).max()
    bar_max, bar_mean = 4 * spread[0] + 1e-6 * top, 2 * spread[1] + 1e-7 * top
    print(f'{what:5s} {name:12s} {v}: max {dd.max():.3e} (bar {bar_max:.3e}, ref {spread[0]:.3e}) mean {dd.mean():.3e} '
          f'(bar {bar_mean:.3e}, ref {spread[1]:.3e}) max|d64| {top:.3e}')
    return dd.max() <= bar_max and dd.mean() <= bar_mean


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_gradient_parity_with_reference_golden(golden, frontends, v):
    """Bars: max |dwav - d64| <= 4 x the reference's own fp32 max spread + 1e-6 max|d64|, mean <= 2 x its mean spread + 1e-7 max|d64|."""
    ok = {}
    for name, d in golden.items():
        e = d[v]
        w = torch.from_numpy(d['wav'])[None].to(DEV)
        got = _dwav(frontends[v], w, [w.shape[1]], torch.from_numpy(e['g'])[None].to(DEV))
        assert got.shape == w.shape and torch.isfinite(got).all()
        ok[name] = _within('grad', name, v, got[0].cpu().numpy(), e['d64'], e['spread'])
    assert all(ok.values()), ok


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_mel_l1_loss_value_and_gradient(golden, v):
    """Value against the reference's F.l1_loss(...) * 45 within 4 x the reference's own fp32-fp64 difference + 1e-6 relative; gradient
    against the fp64 gradient under the bars of the parity test."""
    loss_fn = mel.MelL1Loss(fmax=mh.FMAX[v], device=DEV)
    ok = {}
    for name, d in golden.items():
        e = d[v]
        w = torch.from_numpy(d['wav'])[None].to(DEV).requires_grad_(True)
        loss = loss_fn(w, [w.shape[1]], torch.from_numpy(e['target'])[None].to(DEV))
        assert loss.dim() == 0
        loss.backward()
        ref, f64 = float(e['loss_ref']), float(e['loss64'])
        bar = 4 * abs(ref - f64) + 1e-6 * abs(ref)
        print(f'loss  {name:12s} {v}: {loss.item():.7f} ref {ref:.7f} |diff| {abs(loss.item() - ref):.3e} (bar {bar:.3e})')
        ok[name] = abs(loss.item() - ref) <= bar and _within('dloss', name, v, w.grad[0].cpu().numpy(), e['dloss64'], e['loss_spread'])
    assert all(ok.values()), ok


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_clamped_cells_pass_no_gradient(golden, frontends, v):
    d = golden['sine440']
    lin = gh.lin_fp64(d['wav'], mel.mel_filter_bank(22050, 1024, 80, 0.0, mh.FMAX[v]))
    below = lin < gh.CLIP * (1 - gh.MARGIN)
    assert below.mean() > 0.3                                          # the sine has plenty of clamped cells
    g = np.where(below, np.random.default_rng(5).standard_normal(lin.shape), 0.0).astype(np.float32)
    w = torch.from_numpy(d['wav'])[None].to(DEV)
    got = _dwav(frontends[v], w, [w.shape[1]], torch.from_numpy(g)[None].to(DEV))
    assert torch.count_nonzero(got).item() == 0


BATCH = [33054, 20000, 1000, 513, 512, 511, 385]                      # the ragged batch of test_mel_gpu.py


def _batch(golden):
    speech = torch.from_numpy(golden['speech']['wav'])
    gen = torch.Generator().manual_seed(11)
    S, T = max(BATCH), max(BATCH) // 256
    wavs = torch.full((len(BATCH), S), 1e3)                           # past each row's length: garbage that must never be read
    g = torch.full((len(BATCH), 80, T), float('nan'))                 # past each row's frames: NaN that must never be read
    for b, n in enumerate(BATCH):
        wavs[b, :n] = speech[:n] if b % 2 == 0 else 0.3 * torch.randn(n, generator=gen)
        g[b, :, :n // 256] = torch.randn(80, n // 256, generator=gen)
    return wavs.to(DEV), g.to(DEV)


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_batch_rows_equal_utterances_alone_bitwise(golden, frontends, v):
    fe = frontends[v]
    wavs, g = _batch(golden)
    dwav = _dwav(fe, wavs, BATCH, g)
    assert dwav.shape == wavs.shape and torch.isfinite(dwav).all()
    for b, n in enumerate(BATCH):
        t = n // 256
        assert torch.count_nonzero(dwav[b, n:]).item() == 0, (v, b, n)
        alone = _dwav(fe, wavs[b:b + 1, :n].contiguous(), [n], g[b:b + 1, :, :t].contiguous())
        assert alone.shape == (1, n) and torch.equal(dwav[b, :n], alone[0]), (v, b, n)
        assert torch.count_nonzero(alone).item() > 0
    assert torch.equal(dwav, _dwav(fe, wavs, torch.tensor(BATCH, device=DEV), g))     # lengths as a device tensor
    assert torch.equal(dwav, _dwav(fe, wavs, BATCH, g))                                # a second run


def test_autograd_surface(golden, frontends):
    fe = frontends['hifi']
    wavs, _ = _batch(golden)
    with torch.no_grad():
        plain = fe(wavs, BATCH)
    assert plain[0].grad_fn is None and fe(wavs, BATCH)[0].grad_fn is None            # a waveform without grad: today's path
    w = wavs.clone().requires_grad_(True)
    mels, energy, frames = fe(w, BATCH)
    assert mels.grad_fn is not None and mels.requires_grad
    assert not energy.requires_grad and not frames.requires_grad
    assert torch.equal(mels, plain[0]) and torch.equal(energy, plain[1]) and torch.equal(frames, plain[2])
    with torch.no_grad():
        assert fe(w, BATCH)[0].grad_fn is None                                         # grad mode off


def test_reference_signature_drop_in_back_propagates(golden):
    names = ['speech', 'edge513']
    n = min(len(golden[k]['wav']) for k in names)
    y = torch.stack([torch.from_numpy(golden[k]['wav'][:n]) for k in names]).to(DEV)
    g = torch.randn(2, 80, n // 256, generator=torch.Generator().manual_seed(2)).to(DEV)
    y1 = y.clone().requires_grad_(True)
    got = mel.mel_spectrogram(y1, 1024, 80, 22050, 256, 1024, 0, None, center=False)
    assert got.grad_fn is not None
    got.backward(g)
    want = _dwav(mel.MelSpectrogram(fmax=None, device=DEV), y, [n, n], g)
    assert torch.count_nonzero(want).item() > 0 and torch.equal(y1.grad, want)
    assert mel.mel_spectrogram(y, 1024, 80, 22050, 256, 1024, 0, None).grad_fn is None


def test_ragged_loss_leaves_padding_out_of_sum_and_count(golden):
    loss_fn = mel.MelL1Loss(device=DEV)
    wavs, _ = _batch(golden)
    T = max(BATCH) // 256
    gen = torch.Generator().manual_seed(4)
    target = torch.full((len(BATCH), 80, T), float('nan'))
    for b, n in enumerate(BATCH):
        target[b, :, :n // 256] = torch.randn(80, n // 256, generator=gen) - 5.0
    target = target.to(DEV)
    w = wavs.clone().requires_grad_(True)
    loss = loss_fn(w, BATCH, target)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(w.grad).all()
    total, count = 0.0, 0
    for b, n in enumerate(BATCH):
        t = n // 256
        m = loss_fn.frontend(wavs[b:b + 1, :n].contiguous(), [n])[0][0]
        total += (m.double() - target[b, :, :t].double()).abs().sum().item()
        count += 80 * t
        assert torch.count_nonzero(w.grad[b, n:]).item() == 0
    assert abs(loss.item() - 45.0 * total / count) <= 1e-5 * loss.item()


def test_graph_replay_of_forward_loss_backward_equals_eager_bitwise(golden):
    loss_fn = mel.MelL1Loss(fmax=None, device=DEV)
    wavs, _ = _batch(golden)
    T = max(BATCH) // 256
    target = (torch.randn(len(BATCH), 80, T, generator=torch.Generator().manual_seed(6)) - 5.0).to(DEV)

    def step(w):
        loss = loss_fn(w, BATCH, target)
        return loss, torch.autograd.grad(loss, w)[0]

    static = wavs.clone().requires_grad_(True)
    step(static)                                                     # eager warm-up: packs the operands, caches the lengths
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        outs = step(static)
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):
        new = (0.2 * torch.randn(static.shape, generator=gen)).to(DEV)
        with torch.no_grad():
            static.copy_(new)
        graph.replay()
        ref = step(new.clone().requires_grad_(True))
        for a, b in zip(outs, ref):
            assert torch.equal(a, b)
