"""The kernels of the discriminator step (csrc/dx_disc_wgrad.hip) one by one against float64.

Exact tests: operands that are multiples of 1/4 in [-2, 2], so that every product (a multiple of 1/16, at most 4) and every partial
sum of fewer than 2^18 terms is exact in fp32 whatever the order (every case here has fewer than 10^4): the result must EQUAL float64
``F.conv1d`` autograd, so any indexing, padding, row-boundary or reduction error shows.  Random tests: each element stays within
n_terms * 2^-24 * sum |a| |dz|, the bound of a sum of n_terms exact products accumulated in fp32 in any order."""
import pytest
import torch
import torch.nn.functional as F

from ubisoft_laforge_daft_exprt_amd import discriminators as disc
from ubisoft_laforge_daft_exprt_amd._lib import lib

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24

# the nine layer classes of MPD_LAYERS[1:] and MSD_LAYERS[1:] (the (1024, 1024, 5, 1, 1, 2) layer is in both)
CLASSES = sorted(set(disc.MPD_LAYERS[1:] + disc.MSD_LAYERS[1:]))
MPD_CLASSES = [c for c in CLASSES if c[2] == 5]
MSD_CLASSES = [c for c in CLASSES if c in disc.MSD_LAYERS[1:]]
IDS = lambda c: '-'.join(str(v) for v in c)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dyadic(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 4


def _n_in(n_out, taps, stride, pad, extra=0):
    """The shortest input with n_out output positions, plus ``extra`` (< stride) positions the last window does not reach."""
    return (n_out - 1) * stride + taps - 2 * pad + extra


def _size(rows, n_in, layer):
    cin, cout, taps, stride, groups, pad = layer
    nb, s = torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.int32)
    lib().dx_disc_wgrad_size(rows, n_in, cin, cout, groups, taps, stride, pad, nb.data_ptr(), s.data_ptr())
    return int(nb), int(s)


def _wgrad(a, dz, p, layer):
    """a (Bt, N, p, Cin), dz (Bt, Nout, p, Cout) channels-last as the forward stores them -> (G, dbias) of dx_disc_wgrad."""
    cin, cout, taps, stride, groups, pad = layer
    bt, n_in, n_out = a.shape[0], a.shape[1], dz.shape[1]
    nb, _ = _size(bt * p, n_in, layer)
    ws = torch.full((nb // 4,), float('nan'), device=DEV)                # whatever the reduction reads, the kernel wrote
    G = torch.full((cout, cin // groups, taps), float('nan'), device=DEV)
    db = torch.full((cout,), float('nan'), device=DEV)
    ad, zd = a.to(DEV), dz.to(DEV)
    lib().dx_disc_wgrad(ad.data_ptr(), n_in * p * cin, cin, p * cin, zd.data_ptr(), n_out * p * cout, cout, p * cout, G.data_ptr(), db.data_ptr(),
                        ws.data_ptr(), nb, bt * p, p, n_in, cin, cout, groups, taps, stride, pad, _stream())
    return G.cpu(), db.cpu()


def _reference(a, dz, layer):
    """float64 autograd of F.conv1d over the (batch, column) rows -> (dW (Cout, Cin / groups, taps), db)."""
    cin, cout, taps, stride, groups, pad = layer
    bt, n_in, p, _ = a.shape
    x = a.double().permute(0, 2, 3, 1).reshape(bt * p, cin, n_in)
    g = dz.double().permute(0, 2, 3, 1).reshape(bt * p, cout, -1)
    w = torch.zeros(cout, cin // groups, taps, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    out = F.conv1d(x, w, b, stride=stride, padding=pad, groups=groups)
    assert out.shape == g.shape, (out.shape, g.shape)
    (out * g).sum().backward()
    return w.grad, b.grad


def _operands(g, bt, p, n_in, layer, draw=_dyadic):
    cin, cout, taps, stride, _, pad = layer
    n_out = disc.conv_out(n_in, taps, stride, pad)
    return draw(g, bt, n_in, p, cin), draw(g, bt, n_out, p, cout)


def _check_exact(a, dz, p, layer, what):
    G, db = _wgrad(a, dz, p, layer)
    want_G, want_db = _reference(a, dz, layer)
    assert torch.equal(G.double(), want_G), (what, (G.double() - want_G).abs().max().item())
    assert torch.equal(db.double(), want_db), (what, 'dbias')
    return G, db


@pytest.mark.parametrize('layer', CLASSES, ids=IDS)
def test_wgrad_equals_float64_exactly_across_a_row_boundary(layer):
    """rows = 6 (B = 1, both halves, p = 3) of 70 output positions: the flattened k axis is 6.56 tiles of 64, every tile boundary and
    every row boundary at another offset, and the input has one position more than the last window reaches where the stride allows it
    ((N_in + 2 pad - taps) mod stride != 0).  Twice: the same bits."""
    _, _, taps, stride, _, pad = layer
    g = torch.Generator().manual_seed(sum(layer))
    n_in = _n_in(70, taps, stride, pad, extra=stride - 1)
    assert disc.conv_out(n_in, taps, stride, pad) == 70 and (stride == 1 or (n_in + 2 * pad - taps) % stride != 0)
    a, dz = _operands(g, 2, 3, n_in, layer)
    G, db = _check_exact(a, dz, 3, layer, 'rows 6')
    G2, db2 = _wgrad(a, dz, 3, layer)
    assert torch.equal(G, G2) and torch.equal(db, db2)


@pytest.mark.parametrize('n_in', [1, 2, 3])
@pytest.mark.parametrize('layer', MPD_CLASSES, ids=IDS)
def test_wgrad_with_one_output_position_per_row(layer, n_in):
    """rows = 22 (p = 11) of 1 to 3 input positions: one output position per row in the stride-3 layers (every k entry is a row of its
    own), N_in in the stride-1 layer, and all taps but 1 to 3 read padding."""
    g = torch.Generator().manual_seed(sum(layer) + n_in)
    a, dz = _operands(g, 2, 11, n_in, layer)
    assert dz.shape[1] == (n_in if layer[3] == 1 else 1)
    _check_exact(a, dz, 11, layer, ('rows 22', n_in))


@pytest.mark.parametrize('layer', MSD_CLASSES, ids=IDS)
def test_wgrad_of_the_scale_layers_on_two_rows(layer):
    """rows = 2, p = 1, 33 output positions: a tile that ends inside the second row and a part tile."""
    _, _, taps, stride, _, pad = layer
    g = torch.Generator().manual_seed(sum(layer) + 33)
    a, dz = _operands(g, 2, 1, _n_in(33, taps, stride, pad), layer)
    assert dz.shape[1] == 33
    _check_exact(a, dz, 1, layer, 'rows 2')


@pytest.mark.parametrize('layer', [(128, 128, 41, 2, 4, 20), (32, 128, 5, 3, 1, 2)], ids=IDS)
def test_wgrad_split_into_runs_of_several_tiles(layer):
    """A k axis of 4 x 2400 = 9600 entries, 150 tiles: dx_disc_wgrad_size's rule cuts it into S > 1 runs of more than one tile."""
    _, _, taps, stride, _, pad = layer
    n_in = _n_in(2400, taps, stride, pad)
    _, S = _size(4, n_in, layer)
    assert 1 < S < 150 // 2, S
    g = torch.Generator().manual_seed(sum(layer) + 9600)
    a, dz = _operands(g, 2, 2, n_in, layer)
    G, db = _check_exact(a, dz, 2, layer, 'split')
    G2, db2 = _wgrad(a, dz, 2, layer)
    assert torch.equal(G, G2) and torch.equal(db, db2)


@pytest.mark.parametrize('layer', CLASSES, ids=IDS)
def test_wgrad_on_random_operands_within_the_summation_bound(layer):
    _, _, taps, stride, _, pad = layer
    g = torch.Generator().manual_seed(sum(layer) + 1)
    draw = lambda gen, *shape: torch.randn(shape, generator=gen)
    a, dz = _operands(g, 2, 3, _n_in(70, taps, stride, pad), layer, draw)
    n_terms = 6 * 70
    G, db = _wgrad(a, dz, 3, layer)
    want_G, want_db = _reference(a, dz, layer)
    bound_G, bound_db = _reference(a.abs(), dz.abs(), layer)
    err = (G.double() - want_G).abs()
    print(f'disc wgrad {IDS(layer)}: max err / bound {(err / (n_terms * EPS * bound_G)).max().item():.4f}')
    assert (err <= n_terms * EPS * bound_G).all()
    assert ((db.double() - want_db).abs() <= n_terms * EPS * bound_db).all()


# ---- the seed and conv_post ------------------------------------------------------------------------------------------------------
def _post(score, amap, w, weight, cnt, half_rows, p):
    """score (Bt, N, p), amap (Bt, N, p, C), w (1, C, 3) -> (dZ, dW, db) of dx_disc_post_wgrad."""
    L = lib()
    bt, n, _, C = amap.shape
    nb = torch.zeros(1, dtype=torch.long)
    L.dx_disc_post_wgrad_size(bt * p, n, C, 3, nb.data_ptr())
    ws = torch.full((int(nb) // 8,), float('nan'), dtype=torch.float64, device=DEV)
    sd, ad, wd = score.to(DEV), amap.to(DEV), w.to(DEV)
    gw = torch.tensor([weight], dtype=torch.float32, device=DEV)
    dZ, dW, db = (torch.full(s, float('nan'), device=DEV) for s in (tuple(amap.shape), (1, C, 3), (1,)))
    L.dx_disc_post_wgrad(sd.data_ptr(), n * p, 1, p, wd.data_ptr(), ad.data_ptr(), dZ.data_ptr(), n * p * C, C, p * C, gw.data_ptr(), 2.0 / cnt,
                         dW.data_ptr(), db.data_ptr(), ws.data_ptr(), int(nb), bt * p, half_rows, p, n, C, 3, _stream())
    return dZ.cpu(), dW.cpu(), db.cpu()


def _post_reference(score, amap, w, weight, cnt):
    """float64: the seed of discriminator_loss (real rows first) through conv_post -> (dS, dZ, dW, db)."""
    bt, n, p, C = amap.shape
    half = bt // 2
    s = score.double()
    dS = torch.cat([s[:half] - 1, s[half:]], 0) * (weight * 2.0 / cnt)
    x = amap.double().permute(0, 2, 3, 1).reshape(bt * p, C, n).requires_grad_(True)
    wv = w.double().clone().requires_grad_(True)
    b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    out = F.conv1d(x, wv, b, padding=1)
    (out * dS.permute(0, 2, 1).reshape(bt * p, 1, n)).sum().backward()
    slope = torch.where(amap > 0, torch.tensor(1.0), torch.tensor(0.1, dtype=torch.float32)).double()
    dZ = x.grad.reshape(bt, p, C, n).permute(0, 3, 1, 2)
    return dS, dZ, slope, wv.grad, b.grad


def test_post_wgrad_is_exact_on_dyadic_scores_with_a_power_of_two_count():
    """B = 2 per half, p = 2, N = 4: cnt = 16.  dS = 0.5 (2 / 16) (S - [real]) is a multiple of 1/64 and the sums stay exact, so dW and
    db EQUAL float64, and dZ equals the exact sum times the slope in ONE fp32 rounding (1, or fp32(0.1)).  The real and the generated
    rows differ in their seed: with the halves swapped, or every row seeded as generated, the same call must NOT reproduce them."""
    g = torch.Generator().manual_seed(5)
    bt, n, p, C = 4, 4, 2, 1024
    score, amap, w = _dyadic(g, bt, n, p), _dyadic(g, bt, n, p, C), _dyadic(g, 1, C, 3)
    dZ, dW, db = _post(score, amap, w, 0.5, 16, 2 * p, p)
    dS, want_dZ, slope, want_dW, want_db = _post_reference(score, amap, w, 0.5, 16)
    assert torch.equal(dZ, (want_dZ.float() * slope.float())), (dZ.double() - want_dZ * slope).abs().max()
    assert torch.equal(dW.double(), want_dW) and torch.equal(db.double(), want_db)
    # the generated rows first: another seed, another result
    _, dW_swapped, db_swapped = _post(score, amap, w, 0.5, 16, 0, p)
    assert not torch.equal(dW_swapped, dW) and not torch.equal(db_swapped, db)
    flipped = torch.cat([score[2:], score[:2]], 0), torch.cat([amap[2:], amap[:2]], 0)
    _, dW_f, db_f = _post(*flipped, w, 0.5, 16, 2 * p, p)
    assert not torch.equal(dW_f, dW)


def test_post_wgrad_with_a_count_that_is_no_power_of_two():
    """B = 1 per half, p = 3, N = 7: cnt = 21, so 2 / cnt rounds: every element within the summation bound of its n_terms products
    (each product itself rounded twice more: the seed's scale and its product with the score)."""
    g = torch.Generator().manual_seed(21)
    bt, n, p, C = 2, 7, 3, 1024
    score, amap, w = _dyadic(g, bt, n, p), _dyadic(g, bt, n, p, C), _dyadic(g, 1, C, 3)
    dZ, dW, db = _post(score, amap, w, 1.0, 21, p, p)
    dS, want_dZ, slope, want_dW, want_db = _post_reference(score, amap, w, 1.0, 21)
    n_terms = bt * p * n + 3
    x = amap.double().abs().permute(0, 2, 3, 1).reshape(bt * p, C, n)
    bound_dW = torch.stack([F.pad(x, (1, 1))[:, :, t:t + n].mul(dS.abs().permute(0, 2, 1).reshape(bt * p, 1, n)).sum((0, 2)) for t in range(3)], 1)[None]
    assert ((dW.double() - want_dW).abs() <= n_terms * EPS * bound_dW).all()
    assert abs(float(db) - float(want_db)) <= n_terms * EPS * float(dS.abs().sum())
    bound_dZ = F.conv_transpose1d(dS.abs().permute(0, 2, 1).reshape(bt * p, 1, n), w.double().abs(), padding=1).reshape(bt, p, C, n).permute(0, 3, 1, 2)
    assert ((dZ.double() - want_dZ * slope).abs() <= 8 * EPS * bound_dZ).all()


# ---- the first layer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p,T', [(1, 64), (1, 33), (2, 64), (2, 33), (11, 121), (11, 130)])
def test_first_wgrad_is_exact_through_the_period_view(p, T):
    """Dyadic waveforms; T divisible by p and not (then the reflect tail contributes), against F.conv2d autograd on the padded view."""
    cin, cout, taps, stride, _, pad = disc.MPD_LAYERS[0] if p > 1 else disc.MSD_LAYERS[0]
    g = torch.Generator().manual_seed(p * 1000 + T)
    L = lib()
    R = 4
    x = _dyadic(g, R, T)
    H = -(-T // p)
    hout = disc.conv_out(H, taps, stride, pad)
    dz = _dyadic(g, R, hout, p, cout)
    nb = torch.zeros(1, dtype=torch.long)
    L.dx_disc_first_wgrad_size(R, T, p, cout, taps, stride, pad, nb.data_ptr())
    ws = torch.full((int(nb) // 4,), float('nan'), device=DEV)
    dW, db = torch.full((cout, 1, taps), float('nan'), device=DEV), torch.full((cout,), float('nan'), device=DEV)
    xd, zd = x.to(DEV), dz.to(DEV)
    L.dx_disc_first_wgrad(xd.data_ptr(), T, T, zd.data_ptr(), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), int(nb), R, p, cout, taps, stride, pad,
                          _stream())
    xv = x.double()[:, None]
    if T % p:
        xv = F.pad(xv, (0, p - T % p), 'reflect')
    xv = xv.view(R, 1, H, p)
    w = torch.zeros(cout, 1, taps, 1, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(xv, w, b, stride=(stride, 1), padding=(pad, 0))
    (out * dz.double().permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(dW.cpu().double(), w.grad[..., 0]) and torch.equal(db.cpu().double(), b.grad)


# ---- dx_disc_conv_dgrad over all rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layer', [(128, 512, 5, 3, 1, 2), (256, 512, 41, 4, 16, 20)], ids=IDS)
def test_dgrad_with_a_zero_feature_weight_reduces_to_the_slope(layer):
    """The discriminator step calls dx_disc_conv_dgrad with all 2B rows, R = G = the stored map and gw_fm -> a device zero: the
    epilogue's seed term vanishes (sign(0) = 0) and what is left is the epilogue = 0 result times the slope of the map, bit for bit."""
    cin, cout, taps, stride, groups, pad = layer
    L = lib()
    g = torch.Generator().manual_seed(sum(layer) + 2)
    bt, p, n_in = 4, 3, 40
    n_out = disc.conv_out(n_in, taps, stride, pad)
    w = torch.randn(cout, cin // groups, taps, generator=g).to(DEV)
    nb = torch.zeros(1, dtype=torch.long)
    L.dx_disc_dgrad_pack_size(cin, cout, groups, taps, stride, 0, nb.data_ptr())
    pack = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
    L.dx_disc_dgrad_pack(w.data_ptr(), pack.data_ptr(), cin, cout, groups, taps, stride, 0, _stream())
    amap = torch.randn(bt, n_in, p, cin, generator=g).to(DEV)
    dz = torch.randn(bt, n_out, p, cout, generator=g).to(DEV)
    zero = torch.zeros(1, device=DEV)
    outs = []
    for epi in (0, 1):
        dx = torch.full(tuple(amap.shape), float('nan'), device=DEV)
        L.dx_disc_conv_dgrad(dz.data_ptr(), n_out * p * cout, cout, p * cout, pack.data_ptr(), dx.data_ptr(), amap.data_ptr(), amap.data_ptr(),
                             n_in * p * cin, cin, p * cin, zero.data_ptr(), 2.0 / amap.numel(), bt * p, p, n_in, cin, cout, groups, taps, stride, pad,
                             epi, 0, _stream())
        outs.append(dx)
    slope = torch.where(amap > 0, torch.tensor(1.0, device=DEV), torch.tensor(0.1, dtype=torch.float32, device=DEV))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[1], outs[0] * slope)
