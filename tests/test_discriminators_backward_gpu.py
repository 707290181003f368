"""The discriminators' backward to the generated waveform on the GPU (csrc/dx_disc_bwd.hip).

Two yardsticks.  |r - g| and leaky-ReLU are not smooth, so an fp32 and a float64 forward disagree on a few signs near ties and that,
not rounding, dominates fp32-against-float64 gradient differences.  The HARD bar is therefore on the gradient linearised at the
device's own feature maps (tests/disc_backward_torch.py), under the project's rule with the spread measured here (the same linearised
gradient evaluated by torch in float32 on the CPU, against float64):  max|d| <= 4 spread_max + 1e-6 max|g64|,
mean|d| <= 2 spread_mean + 1e-7 max|g64|.  Against TRUE float64 autograd (and the reference fixture) the bar is statistical: relative
L2 and mean|d| within 4 x torch's own fp32 autograd; max|d| is printed only (which near-tie elements flip decides it).

Per-kernel checks use a-priori bounds: a K-term fp32 dot product in any order errs by at most (K + 2) u32 sum|a w|; bf16 operands add
(2 ubf + ubf^2) sum|a w|; the epilogue (seed product, fused add, slope) four more roundings.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_backward_torch as dbt
from tests import disc_helpers as dh
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U32, UBF = 2.0 ** -24, 2.0 ** -9
WEIGHTS = (1.0, 0.7, 1.3, 0.9)
UNIT = (1.0, 1.0, 1.0, 1.0)


def _lib():
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    return lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cpu_maps(out):
    """(y_d_rs, y_d_gs, fmap_rs, fmap_gs) on the device -> (fmap_rs, fmap_gs) on the CPU."""
    return [[t.cpu() for t in fm] for fm in out[2]], [[t.cpu() for t in fm] for fm in out[3]]


class _Shared:
    def __init__(self):
        states = dh.state_dicts()
        self.states = states
        self.mpd_w = {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]), b) for k, (w, b) in disc.fold_state_dict(states['mpd']).items()}
        self.msd_w = disc.fold_state_dict(states['msd'])
        self.f32 = disc.HiFiGanDiscriminators(states, device=DEV, precision='f32')
        self.bf16 = disc.HiFiGanDiscriminators(states, device=DEV, precision='bf16')
        self._auto, self._hip = {}, {}

    def hip(self, T, precision, weights):
        """-> (the four losses, dy_hat on the CPU in float64, the pass's own (mpd maps, msd maps) on the CPU), computed once."""
        key = (T, precision, weights)
        if key not in self._hip:
            D = getattr(self, precision)
            y, y_hat = (t.to(DEV) for t in dh.inputs(T))
            four, dy = D.generator_loss_grad(y, y_hat, weights)
            dy = dy.cpu().double()
            with torch.no_grad():
                maps = (_cpu_maps(D.mpd(y, y_hat)), _cpu_maps(D.msd(y, y_hat)))
            self._hip[key] = ({k: float(v) for k, v in four.items()}, dy, maps)
        return self._hip[key]

    def autograd(self, T, dtype):
        """True autograd of the restatement at unit weights on the CPU, once."""
        key = (T, dtype)
        if key not in self._auto:
            y, y_hat = dh.inputs(T)
            self._auto[key] = dbt.autograd_grad(y, y_hat, self.mpd_w, self.msd_w, UNIT, dtype)[0].double()
        return self._auto[key]


@pytest.fixture(scope='module')
def S():
    return _Shared()


# ---- per kernel --------------------------------------------------------------------------------------------------------------------------
def _dgrad_pack(w, cin, cout, groups, k, s, bf16):
    n = torch.zeros(1, dtype=torch.long)
    _lib().dx_disc_dgrad_pack_size(cin, cout, groups, k, s, bf16, n.data_ptr())
    buf = torch.empty(int(n.item()), dtype=torch.uint8, device=DEV)
    _lib().dx_disc_dgrad_pack(w.data_ptr(), buf.data_ptr(), cin, cout, groups, k, s, bf16, _st())
    return buf


def _plant_ties(r, g, gen):
    """exact ties in fp32: G == R at a tenth of the elements, G == 0 at another tenth"""
    pick = torch.rand(g.shape, generator=gen)
    g = torch.where(pick < 0.1, r, g)
    return r, torch.where(pick > 0.9, torch.zeros(()), g)


def _epilogue64(acc, seed, r, g):
    r, g = r.double(), g.double()
    one, slope = torch.ones((), dtype=torch.float64), torch.full((), 0.1, dtype=torch.float64)
    return (acc + seed * torch.sign(g - r)) * torch.where(g > 0, one, slope)


DGRAD_CASES = [(32, 128, 1, 5, 3, 2, n, 11) for n in (1, 2, 3, 4, 193)] + [(128, 512, 1, 5, 3, 2, 66, 3), (512, 1024, 1, 5, 3, 2, 7, 2)] + \
              [(128, 128, 4, 41, 2, 20, n, 1) for n in (1, 41, 130)] + \
              [(128, 256, 16, 41, 2, 20, 65, 1), (256, 512, 16, 41, 4, 20, 67, 1), (512, 1024, 16, 41, 4, 20, 70, 1),
               (1024, 1024, 16, 41, 1, 20, 9, 1), (1024, 1024, 1, 5, 1, 2, 3, 1)]


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('cin,cout,groups,k,s,pad,N,p', DGRAD_CASES)
def test_dgrad_kernel_against_float64(cin, cout, groups, k, s, pad, N, p, bf16):
    """dx_disc_conv_dgrad on 3 batch rows (x p columns) against the float64 gradient of F.conv1d, epilogue off and on.  Bound:
    ((K + 4) u32 [+ 2 ubf + ubf^2]) (|dZ| (*)^T |W|), K = ceil(taps / stride) Cout / groups; the epilogue adds 4 u32 (|acc| + |seed|)."""
    gen = torch.Generator().manual_seed(cin * 7 + N)
    B = 3
    nout = disc.conv_out(N, k, s, pad)
    dz = torch.randn(B, nout, p, cout, generator=gen)
    w = torch.randn(cout, cin // groups, k, generator=gen) / math.sqrt(k * cin // groups)
    r, g = _plant_ties(torch.randn(B, N, p, cin, generator=gen), torch.randn(B, N, p, cin, generator=gen), gen)
    gw = torch.tensor([0.7])
    fm_scale = 0.37
    seed = float(gw[0] * torch.tensor(fm_scale))                        # the fp32 product the kernel forms; its rounding is in the bound

    def grad64(dz64, w64):
        x = torch.zeros(B * p, cin, N, dtype=torch.float64, requires_grad=True)
        F.conv1d(x, w64, None, stride=s, padding=pad, groups=groups).backward(dz64.permute(0, 2, 3, 1).reshape(B * p, cout, nout))
        return x.grad.reshape(B, p, cin, N).permute(0, 3, 1, 2)         # (B, N, p, Cin)
    want, mag = grad64(dz.double(), w.double()), grad64(dz.double().abs(), w.double().abs())
    K = -(-k // s) * cout // groups
    bound = ((K + 4) * U32 + (2 * UBF + UBF * UBF if bf16 else 0.0)) * mag
    dzd, wd, rd, gd, gwd = dz.to(DEV), w.to(DEV), r.to(DEV), g.to(DEV), gw.to(DEV)
    pack = _dgrad_pack(wd, cin, cout, groups, k, s, bf16)
    for epi in (0, 1):
        dx = torch.full((B, N, p, cin), float('nan'), device=DEV)
        _lib().dx_disc_conv_dgrad(dzd.data_ptr(), nout * p * cout, cout, p * cout, pack.data_ptr(), dx.data_ptr(), rd.data_ptr(), gd.data_ptr(),
                                  N * p * cin, cin, p * cin, gwd.data_ptr(), fm_scale, B * p, p, N, cin, cout, groups, k, s, pad, epi, bf16, _st())
        got = dx.cpu().double()
        assert torch.isfinite(got).all()
        ref, bnd = (want, bound) if not epi else (_epilogue64(want, seed, r, g), bound + 4 * U32 * (mag + abs(seed)))
        print(f'dgrad {cin}<-{cout} g{groups} k{k} s{s} N={N} bf16={bf16} epilogue={epi}: max|d| {float((got - ref).abs().max()):.3e}, '
              f'max bound {float(bnd.max()):.3e}')
        assert float(((got - ref).abs() - bnd).max()) <= 0


@pytest.mark.parametrize('p', [1, 11])
@pytest.mark.parametrize('N', [1, 2, 3, 9])
def test_post_bwd_kernel(N, p):
    """Score seed + the k 3 transposed product + the epilogue.  dS is formed in fp32 from a handful of operations (8 u32 of its
    magnitude), the product has 3 terms."""
    gen = torch.Generator().manual_seed(N * 10 + p)
    B, C = 3, 1024
    sr, sg = torch.randn(B, N, p, generator=gen), torch.randn(B, N, p, generator=gen)
    sg[0, 0, 0] = sr[0, 0, 0]                                           # a tie: sign(0) = 0
    w = torch.randn(1, C, 3, generator=gen) / 55.0
    r, g = _plant_ties(torch.randn(B, N, p, C, generator=gen), torch.randn(B, N, p, C, generator=gen), gen)
    gw = torch.tensor([1.3, 0.7])
    s_scale, fm_scale = 2.0 / (B * N * p), 2.0 / (B * N * p * C)
    wgen, wfm, seed = float(gw[0] * torch.tensor(s_scale)), float(gw[1] * torch.tensor(s_scale)), float(gw[1] * torch.tensor(fm_scale))
    ds = wgen * (sg.double() - 1) + wfm * torch.sign(sg.double() - sr.double())
    ds_mag = abs(wgen) * (sg.double().abs() + 1) + abs(wfm)

    def grad64(d):
        x = torch.zeros(B * p, C, N, dtype=torch.float64, requires_grad=True)
        F.conv1d(x, w.double().abs() if d is ds_mag else w.double(), None, padding=1).backward(d.permute(0, 2, 1).reshape(B * p, 1, N))
        return x.grad.reshape(B, p, C, N).permute(0, 3, 1, 2)
    want, mag = _epilogue64(grad64(ds), seed, r, g), grad64(ds_mag)
    dz = torch.full((B, N, p, C), float('nan'), device=DEV)
    srg = torch.cat([sr, sg]).to(DEV)
    wd, rd, gd, gwd = w.to(DEV), r.to(DEV), g.to(DEV), gw.to(DEV)
    _lib().dx_disc_post_bwd(srg.data_ptr(), srg.data_ptr() + 4 * B * N * p, N * p, 1, p, wd.data_ptr(), dz.data_ptr(), rd.data_ptr(), gd.data_ptr(),
                            N * p * C, C, p * C, gwd.data_ptr(), gwd.data_ptr() + 4, s_scale, fm_scale, B * p, p, N, C, 3, 1, _st())
    got = dz.cpu().double()
    assert torch.isfinite(got).all()
    assert float(((got - want).abs() - ((3 + 4 + 8) * U32 * mag + 4 * U32 * (mag + abs(seed)))).max()) <= 0


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('T', [12, 257, 2310])
@pytest.mark.parametrize('p', [1, 2, 3, 5, 7, 11])
def test_first_bwd_kernel_gathers_the_period_view_and_the_reflect_mirror(p, T, accumulate):
    """T = 12 and 257 leave a reflect-padded tail for the periods that do not divide them; 2310 = 2 3 5 7 11 has none."""
    gen = torch.Generator().manual_seed(p * 100 + T)
    cout, k, s, pad = (128, 15, 1, 7) if p == 1 else (32, 5, 3, 2)
    B = 3
    H = -(-T // p)
    hout = disc.conv_out(H, k, s, pad)
    dz, w, base = torch.randn(B, hout, p, cout, generator=gen), torch.randn(cout, 1, k, generator=gen), torch.randn(B, T, generator=gen)

    def grad64(d, w64):
        x = torch.zeros(B, 1, T, dtype=torch.float64, requires_grad=True)
        xp = F.pad(x, (0, p - T % p), 'reflect') if T % p else x
        F.conv2d(xp.view(B, 1, H, p), w64[..., None], None, stride=(s, 1), padding=(pad, 0)).backward(d.permute(0, 3, 1, 2))
        return x.grad[:, 0]
    want, mag = grad64(dz.double(), w.double()), grad64(dz.double().abs(), w.double().abs())
    dy = base.to(DEV) if accumulate else torch.full((B, T), float('nan'), device=DEV)
    dzd, wd = dz.to(DEV), w.to(DEV)
    _lib().dx_disc_first_bwd(dzd.data_ptr(), wd.data_ptr(), dy.data_ptr(), T, T, B, p, cout, k, s, pad, accumulate, _st())
    got = dy.cpu().double()
    assert torch.isfinite(got).all()
    if accumulate:
        want, extra = want + base.double(), 2 * U32 * (mag + base.double().abs())
    else:
        extra = 0.0
    assert float(((got - want).abs() - ((2 * k * cout + 4) * U32 * mag + extra)).max()) <= 0


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('T', [1, 2, 3, 4, 7, 12, 257])
def test_pool_bwd_kernel(T, accumulate):
    gen = torch.Generator().manual_seed(T)
    dy, base = torch.randn(3, T // 2 + 1, generator=gen), torch.randn(3, T, generator=gen)

    def grad64(d):
        x = torch.zeros(3, 1, T, dtype=torch.float64, requires_grad=True)
        F.avg_pool1d(x, 4, 2, padding=2).backward(d[:, None])
        return x.grad[:, 0]
    want, mag = grad64(dy.double()), grad64(dy.double().abs())
    dx = base.to(DEV) if accumulate else torch.full((3, T), float('nan'), device=DEV)
    dyd = dy.to(DEV)
    _lib().dx_disc_pool_bwd(dyd.data_ptr(), dx.data_ptr(), 3, T, accumulate, _st())
    got = dx.cpu().double()
    if accumulate:
        want, mag = want + base.double(), mag + base.double().abs()
    assert float(((got - want).abs() - 4 * U32 * mag).max()) <= 0


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', dh.LENGTHS)
def test_f32_gradient_linearised_at_the_device_maps(S, T):
    """The hard bar.  Measured on the MI355X (error / bar, max and mean): see DESIGN §15."""
    four, dy, (mpd_maps, msd_maps) = S.hip(T, 'f32', WEIGHTS)
    y_hat = dh.inputs(T)[1]
    g64 = dbt.linearised_grad(y_hat, S.mpd_w, S.msd_w, mpd_maps, msd_maps, WEIGHTS, torch.float64)
    g32 = dbt.linearised_grad(y_hat, S.mpd_w, S.msd_w, mpd_maps, msd_maps, WEIGHTS, torch.float32).double()
    spread, d = (g32 - g64).abs(), (dy - g64).abs()
    scale = float(g64.abs().max())
    bmax, bmean = 4 * float(spread.max()) + 1e-6 * scale, 2 * float(spread.mean()) + 1e-7 * scale
    print(f'linearised T={T}: max|g64| {scale:.4f}; max|d| {float(d.max()):.3e} (bar {bmax:.3e}, ratio {float(d.max()) / bmax:.2f}); '
          f'mean|d| {float(d.mean()):.3e} (bar {bmean:.3e}, ratio {float(d.mean()) / bmean:.2f}); torch fp32 spread max '
          f'{float(spread.max()):.3e} mean {float(spread.mean()):.3e}')
    assert dy.shape == g64.shape and torch.isfinite(dy).all()
    assert float(d.max()) <= bmax and float(d.mean()) <= bmean


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_f32_gradient_against_true_autograd_and_the_reference_fixture(S, T):
    z = dbt.fixture()
    four, dy, _ = S.hip(T, 'f32', UNIT)
    bad = []
    for what, g64, g32 in (('autograd', S.autograd(T, torch.float64), S.autograd(T, torch.float32)),
                           ('fixture', torch.from_numpy(z[f'{T}/grad64']), torch.from_numpy(z[f'{T}/grad32']).double())):
        rel = lambda a: float((a - g64).norm() / g64.norm())
        mean = lambda a: float((a - g64).abs().mean())
        print(f'{what} T={T}: relative L2 {rel(dy):.3e} (torch fp32 {rel(g32):.3e}, ratio {rel(dy) / rel(g32):.2f}); mean|d| {mean(dy):.3e} '
              f'(torch fp32 {mean(g32):.3e}, ratio {mean(dy) / mean(g32):.2f}); max|d| {float((dy - g64).abs().max()):.3e} '
              f'(torch fp32 {float((g32 - g64).abs().max()):.3e}), max|g64| {float(g64.abs().max()):.4f}')
        if rel(dy) > 4 * rel(g32) or mean(dy) > 4 * mean(g32):
            bad.append((what, rel(dy), rel(g32), mean(dy), mean(g32)))
    want = z[f'{T}/losses64']                                          # the names map to the right totals (parity proper: the forward tests)
    for v, name in zip(want, disc.GEN_LOSS_NAMES):
        assert abs(four[name] - v) <= 1e-4 * abs(v), name
    assert not bad, bad


def _snr(x, ref):
    noise = float(((x - ref) ** 2).sum())
    return math.inf if noise == 0 else 10 * math.log10(float((ref ** 2).sum()) / noise)


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_bf16_gradient_snr_against_the_emulated_bf16_chain(S, T):
    """Device bf16 against the float64 helper linearised at the bf16 pass's maps with bf16-rounded weights: at least the SNR of the same
    helper with dZ rounded to bf16 at the MFMA layers, minus 3 dB (the forward's rule)."""
    _, dy, (mpd_maps, msd_maps) = S.hip(T, 'bf16', WEIGHTS)
    y_hat = dh.inputs(T)[1]
    ref = dbt.linearised_grad(y_hat, S.mpd_w, S.msd_w, mpd_maps, msd_maps, WEIGHTS, torch.float64, operand='bf16')
    emu = dbt.linearised_grad(y_hat, S.mpd_w, S.msd_w, mpd_maps, msd_maps, WEIGHTS, torch.float64, operand='bf16', round_grad=True)
    got, want = _snr(dy, ref), _snr(emu, ref)
    print(f'bf16 gradient SNR T={T}: HIP bf16 {got:.1f} dB, emulated bf16 chain {want:.1f} dB')
    assert torch.isfinite(dy).all() and got >= want - 3.0


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------
def test_autograd_gives_the_bits_of_generator_loss_grad(S):
    T = 257
    D = S.f32
    y, y_hat = (t.to(DEV) for t in dh.inputs(T))
    with torch.no_grad():
        six = {k: v.clone() for k, v in D.losses(y, y_hat).items()}
    four, want = D.generator_loss_grad(y, y_hat, WEIGHTS)
    assert sorted(four) == sorted(disc.GEN_LOSS_NAMES) and want.shape == y_hat.shape
    assert all(v.dim() == 0 and v.is_cuda and torch.equal(v, six[k]) for k, v in four.items())
    want = want.clone()
    assert torch.equal(D.generator_loss_grad(y, y_hat, torch.tensor(WEIGHTS, device=DEV))[1], want)     # a device tensor of 4
    x = y_hat.clone().requires_grad_(True)
    out = D.generator_losses(y, x)
    assert all(torch.equal(out[k], six[k]) and out[k].requires_grad for k in disc.GEN_LOSS_NAMES)
    (got,) = torch.autograd.grad(sum(w * out[k] for w, k in zip(WEIGHTS, disc.GEN_LOSS_NAMES)), x)
    assert torch.equal(got, want)
    # one loss alone: the other three upstream gradients are None and count as 0
    for i, name in enumerate(disc.GEN_LOSS_NAMES):
        (got,) = torch.autograd.grad(D.generator_losses(y, x)[name], x)
        alone = D.generator_loss_grad(y, y_hat, tuple(1.0 if j == i else 0.0 for j in range(4)))[1]
        assert torch.equal(got, alone) and torch.count_nonzero(got).item() > 0, name
    assert x.grad is None and not y.requires_grad


def test_a_second_pass_before_backward_raises(S):
    T = 257
    D = S.f32
    y, y_hat = (t.to(DEV) for t in dh.inputs(T))
    x = y_hat.clone().requires_grad_(True)
    out = D.generator_losses(y, x)
    with torch.no_grad():
        D.losses(y, y_hat)                                             # the same (B, T): the plan's maps are overwritten
    with pytest.raises(RuntimeError, match='overwritten by a later pass'):
        out['loss_fm_f'].backward()
    out = D.generator_losses(y, x)
    with torch.no_grad():
        D.losses(y[:1], y_hat[:1])                                     # another shape has a plan of its own
    out['loss_fm_f'].backward()
    assert torch.isfinite(x.grad).all()
    with pytest.raises(RuntimeError, match='y must not require grad'):
        D.generator_losses(x, y_hat)


def test_one_backward_adds_the_mel_and_the_adversarial_gradients(S):
    from ubisoft_laforge_daft_exprt_amd import mel
    T = 2048
    D = S.f32
    y, y_hat = (t.to(DEV) for t in dh.inputs(T))
    B = y.shape[0]
    loss_fn = mel.MelL1Loss(fmax=None, device=DEV)
    target = (torch.randn(B, 80, T // 256, generator=torch.Generator().manual_seed(3)) - 5.0).to(DEV)
    x = y_hat.clone().requires_grad_(True)
    (g_mel,) = torch.autograd.grad(loss_fn(x[:, 0], [T] * B, target), x)
    g_adv = D.generator_loss_grad(y, y_hat, UNIT)[1]
    adv = D.generator_losses(y, x)
    total = loss_fn(x[:, 0], [T] * B, target) + adv['loss_gen_s'] + adv['loss_gen_f'] + adv['loss_fm_s'] + adv['loss_fm_f']
    total.backward()
    assert torch.count_nonzero(g_mel).item() > 0 and torch.count_nonzero(g_adv).item() > 0
    assert torch.equal(x.grad, g_mel + g_adv)


# ---- determinism and isolation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_runs_rows_and_a_graph_replay_are_bitwise_stable(S, precision):
    D = getattr(S, precision)
    T = 257
    y, y_hat = (t.to(DEV) for t in dh.make_inputs(T, 77, batch=3))
    y2, y2_hat = (t.to(DEV) for t in dh.make_inputs(T, 78, batch=3))
    first = D.generator_loss_grad(y, y_hat, WEIGHTS)[1].clone()
    assert torch.equal(D.generator_loss_grad(y, y_hat, WEIGHTS)[1], first)                       # two runs
    ym, ym_hat = y.clone(), y_hat.clone()
    ym[1], ym_hat[1] = y2[1], y2_hat[1]
    mixed = D.generator_loss_grad(ym, ym_hat, WEIGHTS)[1]
    assert torch.equal(mixed[0], first[0]) and torch.equal(mixed[2], first[2]) and not torch.equal(mixed[1], first[1])
    eager = D.generator_loss_grad(y2, y2_hat, WEIGHTS)[1].clone()
    sy, sy_hat = y.clone(), y_hat.clone()
    D.generator_loss_grad(sy, sy_hat, WEIGHTS)                                                   # the eager call before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        four, dy = D.generator_loss_grad(sy, sy_hat, WEIGHTS)
    sy.copy_(y2)
    sy_hat.copy_(y2_hat)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dy, eager)
    with torch.no_grad():
        six = D.losses(y2, y2_hat)
    assert all(torch.equal(four[k], six[k]) for k in four)
