"""HiFi-GAN discriminators on the GPU (csrc/dx_disc.hip) against the plain-torch restatement in float64 (tests/disc_torch.py).

The parity rule is the project's, with the reference's own fp32-against-fp64 spreads from the fixture:
per feature map  max|d| <= 4 spread_max + 1e-6 max|f64|  and  mean|d| <= 2 spread_mean + 1e-7 max|f64|;  per loss
|d| <= 4 spread + 1e-6 |f64|.

Measured on the MI355X: the worst error / bar over all maps is 0.40 (the MPD scores at T = 2048, mean|d| 1.3e-8 against
3.3e-8); the feature maps proper stay below 0.2.  With the K sum of dx_disc_conv as ONE MFMA chain the scores missed the mean bar
(1.5 at T = 2048, 1.07 at T = 12); the sum is therefore blocked (64 products per chain in f32).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import disc_helpers as dh
from tests import disc_torch
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U32, UBF = 2.0 ** -24, 2.0 ** -9          # unit roundoffs of fp32 and bf16 (round to nearest)


class _Shared:
    def __init__(self):
        states = dh.state_dicts()
        self.states = states
        self.folded = {'mpd': {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]), b) for k, (w, b) in disc.fold_state_dict(states['mpd']).items()},
                       'msd': disc.fold_state_dict(states['msd'])}
        self.f32 = disc.HiFiGanDiscriminators(states, device=DEV, precision='f32')
        self.bf16 = disc.HiFiGanDiscriminators(states, device=DEV, precision='bf16')
        self._ref, self._hip = {}, {}

    def ref(self, T, operand='f32'):
        """The float64 restatement's (mpd outputs, msd outputs) on the fixture inputs of length T, computed once on the CPU."""
        key = (T, operand)
        if key not in self._ref:
            y, y_hat = dh.inputs(T)
            with torch.no_grad():
                self._ref[key] = (disc_torch.mpd(y, y_hat, self.folded['mpd'], torch.float64, operand),
                                  disc_torch.msd(y, y_hat, self.folded['msd'], torch.float64, operand))
        return self._ref[key]

    def hip(self, T, precision):
        key = (T, precision)
        if key not in self._hip:
            y, y_hat = (t.to(DEV) for t in dh.inputs(T))
            D = getattr(self, precision)
            with torch.no_grad():
                self._hip[key] = (D.mpd(y, y_hat), D.msd(y, y_hat))
        return self._hip[key]


@pytest.fixture(scope='module')
def S():
    return _Shared()


def _maps(out):
    """(y_d_rs, y_d_gs, fmap_rs, fmap_gs) -> [(sub, map, r, g)]"""
    return [(i, j, r, g) for i, (fr, fg) in enumerate(zip(out[2], out[3])) for j, (r, g) in enumerate(zip(fr, fg))]


def _cat64(r, g):
    return torch.cat([r.detach().double().cpu().flatten(), g.detach().double().cpu().flatten()])


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_f32_parity_of_every_feature_map_and_score(S, T):
    z = dh.fixture()
    worst, layer = {}, {}
    bad = []
    for d, hip, ref in zip(('mpd', 'msd'), S.hip(T, 'f32'), S.ref(T)):
        for k in (0, 1):                                              # the scores are the last feature map, flattened
            for i, (a, b) in enumerate(zip(hip[k], ref[k])):
                assert a.shape == b.shape and torch.equal(a.flatten(), hip[2 + k][i][-1].flatten())
        for (i, j, r, g), (_, _, r64, g64) in zip(_maps(hip), _maps(ref)):
            assert r.shape == r64.shape and g.shape == g64.shape, (d, i, j)
            st = z[f'{T}/{d}/{i}/fmap{j}/stats']
            diff = (_cat64(r, g) - _cat64(r64, g64)).abs()
            mx, mean = float(diff.max()), float(diff.mean())
            bmx, bmean = 4 * st[4] + 1e-6 * st[6], 2 * st[5] + 1e-7 * st[6]
            ratio = max(mx / bmx, mean / bmean)
            if ratio > worst.get(d, (0,))[0]:
                worst[d] = (ratio, i, j, mx, bmx, mean, bmean)
            if mx > bmx or mean > bmean:
                bad.append((d, i, j, mx, bmx, mean, bmean))
            layer[(d, j)] = max(layer.get((d, j), 0.0), ratio)
    for d, (ratio, i, j, mx, bmx, mean, bmean) in worst.items():
        print(f'f32 parity T={T} {d}: worst map sub {i} layer {j}: max {mx:.3e} (bound {bmx:.3e}) mean {mean:.3e} (bound {bmean:.3e})')
    print(f'f32 parity T={T}: worst error / bound per layer: ' + ', '.join(f'{d}{j} {v:.2f}' for (d, j), v in sorted(layer.items())))
    assert not bad, bad


def _snr(x, ref):
    noise = float(((x - ref) ** 2).sum())
    return math.inf if noise == 0 else 10 * math.log10(float((ref ** 2).sum()) / noise)


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_bf16_snr_against_the_emulated_bf16_restatement(S, T):
    bad, low = [], {}
    for d, hb, hf, eb, ef in zip(('mpd', 'msd'), S.hip(T, 'bf16'), S.hip(T, 'f32'), S.ref(T, 'bf16'), S.ref(T)):
        for (i, j, rb, gb), (_, _, rf, gf), (_, _, reb, geb), (_, _, ref_r, ref_g) in zip(_maps(hb), _maps(hf), _maps(eb), _maps(ef)):
            got, want = _snr(_cat64(rb, gb), _cat64(rf, gf)), _snr(_cat64(reb, geb), _cat64(ref_r, ref_g))
            if got < low.get(d, (math.inf,))[0]:
                low[d] = (got, want, i, j)
            if got < want - 3.0:
                bad.append((d, i, j, got, want))
    for d, (got, want, i, j) in low.items():
        print(f'bf16 SNR T={T} {d}: lowest map sub {i} layer {j}: HIP bf16 vs HIP f32 {got:.1f} dB, emulated bf16 vs f64 {want:.1f} dB')
    assert not bad, bad


# ---- per-kernel checks ---------------------------------------------------------------------------------------------------------------
def _pack(w, bf16):
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    cout, cin_g, k = w.shape
    n = torch.zeros(1, dtype=torch.long)
    lib().dx_disc_pack_size(cout, cin_g, k, bf16, n.data_ptr())
    buf = torch.empty(int(n.item()), dtype=torch.uint8, device=DEV)
    lib().dx_disc_pack(w.data_ptr(), buf.data_ptr(), cout, cin_g, k, bf16, torch.cuda.current_stream().cuda_stream)
    return buf


CONV_CASES = [(32, 128, 1, 5, 3, 2, n, 11) for n in (1, 2, 3, 193)] + [(128, 128, 4, 41, 2, 20, n, 1) for n in (1, 41, 129)] + \
             [(128, 256, 16, 41, 2, 20, 65, 1), (256, 512, 16, 41, 4, 20, 67, 1), (1024, 1024, 16, 41, 1, 20, 9, 1), (1024, 1024, 1, 5, 1, 2, 3, 1)]


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('cin,cout,groups,k,s,pad,N,p', CONV_CASES)
def test_conv_kernel_against_float64(cin, cout, groups, k, s, pad, N, p, bf16):
    """dx_disc_conv against F.conv1d in float64 on 3 batch rows (x p columns in the MPD layout, where the conv runs along H for each
    column).  Bound, a priori: a K-term fp32 dot product in any order errs by at most (K + 2) u32 sum|a w|; bf16 operands add
    (2 ubf + ubf^2) sum|a w|; bias add and leaky-ReLU two more roundings."""
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    g = torch.Generator().manual_seed(cin * 7 + N)
    B = 3
    x = torch.randn(B, N, p, cin, generator=g)
    w = torch.randn(cout, cin // groups, k, generator=g) / math.sqrt(k * cin // groups)
    b = torch.randn(cout, generator=g)
    nout = disc.conv_out(N, k, s, pad)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = torch.full((B, nout, p, cout), float('nan'), device=DEV)
    lib().dx_disc_conv(xd.data_ptr(), N * p * cin, cin, p * cin, _pack(wd, bf16).data_ptr(), bd.data_ptr(), y.data_ptr(), nout * p * cout, cout,
                       p * cout, B * p, p, N, cin, cout, groups, k, s, pad, 1, bf16, torch.cuda.current_stream().cuda_stream)
    x64 = x.double().permute(0, 2, 3, 1).reshape(B * p, cin, N)                         # (rows, C, N)
    lin = F.conv1d(x64, w.double(), b.double(), stride=s, padding=pad, groups=groups)
    want = F.leaky_relu(lin, 0.1)
    mag = F.conv1d(x64.abs(), w.double().abs(), b.double().abs(), stride=s, padding=pad, groups=groups)
    K = k * cin // groups
    bound = ((K + 4) * U32 + (2 * UBF + UBF * UBF if bf16 else 0.0)) * mag
    got = y.cpu().double().permute(0, 2, 3, 1).reshape(B * p, cout, nout)
    assert torch.isfinite(got).all()
    excess = ((got - want).abs() - bound).max()
    print(f'conv {cin}->{cout} g{groups} k{k} s{s} N={N} bf16={bf16}: max|d| {float((got - want).abs().max()):.3e}, max bound {float(bound.max()):.3e}')
    assert float(excess) <= 0


@pytest.mark.parametrize('p,T', [(2, 8), (2, 9), (11, 22), (11, 23), (11, 32), (1, 37)])
def test_first_layer_kernel_reads_the_period_view_with_reflect_padding(p, T):
    """T mod p in {0, 1, p - 1}: no padding, the longest (p - 1 samples) and the shortest (1 sample) reflect padding."""
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    g = torch.Generator().manual_seed(p * 100 + T)
    cout, k, s, pad = (128, 15, 1, 7) if p == 1 else (32, 5, 3, 2)
    B = 3
    x, w, b = torch.randn(B, 1, T, generator=g), torch.randn(cout, 1, k, generator=g), torch.randn(cout, generator=g)
    H = -(-T // p)
    hout = disc.conv_out(H, k, s, pad)
    y = torch.full((B, hout, p, cout), float('nan'), device=DEV)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    lib().dx_disc_first(xd.data_ptr(), T, T, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, p, cout, k, s, pad, torch.cuda.current_stream().cuda_stream)
    x64 = x.double()
    if T % p:
        x64 = F.pad(x64, (0, p - T % p), 'reflect')
    x64 = x64.view(B, 1, H, p)
    want = F.leaky_relu(F.conv2d(x64, w.double()[..., None], b.double(), stride=(s, 1), padding=(pad, 0)), 0.1)
    mag = F.conv2d(x64.abs(), w.double().abs()[..., None], b.double().abs(), stride=(s, 1), padding=(pad, 0))
    got = y.cpu().double().permute(0, 3, 1, 2)
    assert float(((got - want).abs() - (k + 4) * U32 * mag).max()) <= 0


@pytest.mark.parametrize('T', [1, 2, 7])
def test_pool_kernel(T):
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    x = torch.randn(3, T, generator=torch.Generator().manual_seed(T))
    xd = x.to(DEV)
    y = torch.full((3, T // 2 + 1), float('nan'), device=DEV)
    lib().dx_disc_pool(xd.data_ptr(), y.data_ptr(), 3, T, torch.cuda.current_stream().cuda_stream)
    want = F.avg_pool1d(x.double()[:, None], 4, 2, padding=2)[:, 0]
    assert want.shape == y.shape
    mag = F.avg_pool1d(x.double().abs()[:, None], 4, 2, padding=2)[:, 0]
    assert float(((y.cpu().double() - want).abs() - 4 * U32 * mag).max()) <= 0


@pytest.mark.parametrize('N,p', [(1, 1), (2, 1), (1, 3), (2, 3)])
def test_post_kernel(N, p):
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    g = torch.Generator().manual_seed(N * 10 + p)
    B, C = 3, 1024
    x, w, b = torch.randn(B, N, p, C, generator=g), torch.randn(1, C, 3, generator=g) / 55.0, torch.randn(1, generator=g)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = torch.full((B, N, p), float('nan'), device=DEV)
    lib().dx_disc_post(xd.data_ptr(), N * p * C, C, p * C, wd.data_ptr(), bd.data_ptr(), y.data_ptr(), N * p, 1, p, B * p, p, N, C, 3,
                       torch.cuda.current_stream().cuda_stream)
    x64 = x.double().permute(0, 2, 3, 1).reshape(B * p, C, N)
    want = F.conv1d(x64, w.double(), b.double(), padding=1)
    mag = F.conv1d(x64.abs(), w.double().abs(), b.double().abs(), padding=1)
    got = y.cpu().double().permute(0, 2, 1).reshape(B * p, 1, N)
    assert float(((got - want).abs() - (3 * C + 4) * U32 * mag).max()) <= 0


# ---- bitwise properties ----------------------------------------------------------------------------------------------------------------
def _flat(out):
    return [t for t in out[0] + out[1]] + [t for fm in out[2] + out[3] for t in fm]


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_batch_rows_runs_and_the_real_half_are_bitwise_stable(S, precision):
    D = getattr(S, precision)
    T = 257
    y, y_hat = (t.to(DEV) for t in dh.make_inputs(T, 77, batch=3))
    _, other = (t.to(DEV) for t in dh.make_inputs(T, 78, batch=3))
    with torch.no_grad():
        for m in (D.mpd, D.msd):
            full, again, swapped = m(y, y_hat), m(y, y_hat), m(y, other)
            for a, b in zip(_flat(full), _flat(again)):
                assert torch.equal(a, b)                                              # two runs
            for a, b in zip(full[0] + [t for fm in full[2] for t in fm], swapped[0] + [t for fm in swapped[2] for t in fm]):
                assert torch.equal(a, b)                                              # fmap_r does not depend on y_hat
            assert not torch.equal(full[1][0], swapped[1][0])
            for row in range(3):
                alone = m(y[row:row + 1], y_hat[row:row + 1])
                for a, b in zip(_flat(full), _flat(alone)):
                    assert torch.equal(a[row:row + 1], b)                             # a batch row is the row run alone


# ---- losses ----------------------------------------------------------------------------------------------------------------------------
def _loss_spreads(T):
    """{name: reference |f32 - f64|} of the six totals, from the fixture."""
    z = dh.fixture()
    out = {}
    for d, tag in (('mpd', 'f'), ('msd', 's')):
        for kind in ('disc', 'gen', 'fm'):
            out[f'loss_{kind}_{tag}'] = abs(z[f'{T}/{d}/loss/f32/{kind}'][0] - z[f'{T}/{d}/loss/f64/{kind}'][0])
    return out


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_losses_against_float64(S, T):
    z = dh.fixture()
    y, y_hat = (t.to(DEV) for t in dh.inputs(T))
    with torch.no_grad():
        got = {k: float(v) for k, v in S.f32.losses(y, y_hat).items()}
    assert sorted(got) == sorted(disc.LOSS_NAMES)
    spreads = _loss_spreads(T)
    # (a) the loss kernel alone: float64 sums of the SAME HIP feature maps and scores
    own = disc_torch.six_losses(*[tuple([t.double().cpu() for t in part] if k < 2 else [[t.double().cpu() for t in fm] for fm in part]
                                        for k, part in enumerate(out)) for out in S.hip(T, 'f32')])
    # (b) end to end: the float64 restatement
    ref = disc_torch.six_losses(*S.ref(T))
    bad = []
    for name in disc.LOSS_NAMES:
        for what, want in (('kernel', float(own[name])), ('end to end', float(ref[name]))):
            d, bound = abs(got[name] - want), 4 * spreads[name] + 1e-6 * abs(want)
            print(f'loss T={T} {name} {what}: {got[name]:.7f} vs {want:.7f}: |d| {d:.2e} (bound {bound:.2e})')
            if d > bound:
                bad.append((name, what, d, bound))
    # the per-sub-discriminator terms, kernel alone, with the fixture's per-term spreads
    with torch.no_grad():
        for d, hip in zip(('mpd', 'msd'), S.hip(T, 'f32')):
            dl, rl, gl = disc.discriminator_loss(hip[0], hip[1])
            gen, gens = disc.generator_loss(hip[1])
            assert all(t.dim() == 0 and t.is_cuda for t in [dl, gen] + rl + gl + gens)
            o64 = [[t.double().cpu() for t in part] for part in hip[:2]]
            dl64, rl64, gl64 = disc_torch.discriminator_loss(*o64)
            gen64, gens64 = disc_torch.generator_loss(o64[1])
            for tag, a, b in (('disc', [dl] + rl + gl, [dl64] + rl64 + gl64), ('gen', [gen] + gens, [gen64] + gens64)):
                spread = np.abs(z[f'{T}/{d}/loss/f32/{tag}'] - z[f'{T}/{d}/loss/f64/{tag}'])
                for n, (u, v) in enumerate(zip(a, b)):
                    if abs(float(u) - float(v)) > 4 * spread[n] + 1e-6 * abs(float(v)):
                        bad.append((d, tag, n, float(u), float(v)))
    assert not bad, bad


def test_reference_signature_losses_give_the_bits_of_losses(S):
    T = 257
    y, y_hat = (t.to(DEV) for t in dh.inputs(T))
    with torch.no_grad():
        six = S.f32.losses(y, y_hat)
        for tag, out in zip(('f', 's'), S.hip(T, 'f32')):
            dl, rl, gl = disc.discriminator_loss(out[0], out[1])
            gen, gens = disc.generator_loss(out[1])
            fm = disc.feature_loss(out[2], out[3])
            assert torch.equal(dl, six[f'loss_disc_{tag}']) and torch.equal(gen, six[f'loss_gen_{tag}']) and torch.equal(fm, six[f'loss_fm_{tag}'])
            assert len(rl) == len(gl) == len(gens) == len(out[0])
            assert all(t.dim() == 0 and t.is_cuda for t in rl + gl + gens)
        again = S.f32.losses(y, y_hat)
        assert all(torch.equal(six[k], again[k]) for k in six)


def test_losses_replay_from_a_captured_graph(S):
    T = 257
    y, y_hat = (t.to(DEV) for t in dh.make_inputs(T, 5))
    y2, y2_hat = (t.to(DEV) for t in dh.make_inputs(T, 6))
    with torch.no_grad():
        eager = {k: v.clone() for k, v in S.f32.losses(y2, y2_hat).items()}
        sy, sy_hat = y.clone(), y_hat.clone()
        S.f32.losses(sy, sy_hat)                                                       # the eager call that builds the plan
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = S.f32.losses(sy, sy_hat)
        sy.copy_(y2)
        sy_hat.copy_(y2_hat)
        graph.replay()
        torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(out[k], eager[k]), k
