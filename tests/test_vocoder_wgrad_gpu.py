"""The kernels of the generator's backward (csrc/dx_vocoder_bwd.hip) one by one against float64.

Rows: B = 2 with 70 and 33 valid positions of N = 70 -- one whole 64-position tile plus a part, and a row that is masked from position
33 on; the upstream gradient is random over the masked positions too, and nothing may leak from there.  Exact tests: operands that are
multiples of 1/4 in [-2, 2], so that every product (a multiple of 1/16, at most 4) and every partial sum of the at most 103 terms is
exact in fp32 whatever the order: the result must EQUAL float64, so any indexing, masking or reduction error shows.  Leaky-ReLU tests:
the operand is a = fp32(x * fp32(0.1)) as the device stages it, and each element stays within n_terms * 2^-24 * sum |a| |dy|, the
bound of a sum of n_terms exact products accumulated in fp32 in any order (each of the n_terms - 1 additions rounds a partial sum that
is at most sum |a| |dy|, to relative 2^-24)."""
import pytest
import torch

from tests import vocoder_backward_helpers as H
from ubisoft_laforge_daft_exprt_amd._lib import lib

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

B, N, ROWS = 2, 70, (70, 33)
WIDTHS = ((16, 16), (32, 16), (64, 128))                  # (Cin, Cout)
PAIRS = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)] + [(3, 2), (5, 2), (5, 6), (7, 12)]     # V1 / V2's, then V3's ((3, 1) and (7, 3) are in both)
EPS = 2.0 ** -24


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dyadic(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float() / 4


def _frames(scale=1, rows=ROWS):
    return torch.tensor([r // scale for r in rows], dtype=torch.int32, device=DEV)


def _wgrad(x, strides, dy, cin, cout, taps, dil, up, act, n=N, rows=ROWS):
    """x, dy: device tensors -> (G, dbias) of dx_voc_wgrad on B rows of n positions."""
    L = lib()
    nb = torch.zeros(1, dtype=torch.long)
    L.dx_voc_wgrad_size(B, n, cin, cout, taps, up, nb.data_ptr())
    ws = torch.full((int(nb) // 4,), float('nan'), device=DEV)           # whatever the reduction reads, the kernel wrote
    G = torch.full((cin, cout, 2 * up) if up > 1 else (cout, cin, taps), float('nan'), device=DEV)
    db = torch.full((cout,), float('nan'), device=DEV)
    L.dx_voc_wgrad(x.data_ptr(), *strides, dy.data_ptr(), n * up * cout, up * cout, 0, G.data_ptr(), db.data_ptr(), ws.data_ptr(), int(nb),
                   _frames(1, rows).data_ptr(), 1, B, n, cin, cout, taps, dil, up, act, _stream())
    return G.cpu(), db.cpu()


def _masked(t, up=1, rows=ROWS):
    return H._mask(t.double(), list(rows), up)


def _check_exact(x, dy, G, db, taps, dil, up, what):
    want_G, want_db = H.wgrad_reference(_masked(x), _masked(dy, up), taps, dil, up, 0)
    assert torch.equal(G.double(), want_G), (what, (G.double() - want_G).abs().max().item())
    assert torch.equal(db.double(), want_db), (what, 'dbias')


@pytest.mark.parametrize('taps,dil', PAIRS)
def test_wgrad_equals_float64_exactly_on_dyadic_operands(taps, dil):
    g = torch.Generator().manual_seed(taps * 100 + dil)
    for cin, cout in WIDTHS:
        x, dy = _dyadic(g, B, N, cin), _dyadic(g, B, N, cout)
        G, db = _wgrad(x.to(DEV), (N * cin, cin, 1), dy.to(DEV), cin, cout, taps, dil, 1, 0)
        _check_exact(x, dy, G, db, taps, dil, 1, (cin, cout))
        G2, db2 = _wgrad(x.to(DEV), (N * cin, cin, 1), dy.to(DEV), cin, cout, taps, dil, 1, 0)
        assert torch.equal(G, G2) and torch.equal(db, db2)


@pytest.mark.parametrize('taps,dil', PAIRS)
def test_wgrad_with_leaky_relu_within_the_summation_bound(taps, dil):
    g = torch.Generator().manual_seed(taps * 100 + dil + 7)
    slope = torch.tensor(0.1, dtype=torch.float32)
    n_terms = sum(ROWS)
    for cin, cout in WIDTHS:
        x, dy = torch.randn(B, N, cin, generator=g), torch.randn(B, N, cout, generator=g)
        G, db = _wgrad(x.to(DEV), (N * cin, cin, 1), dy.to(DEV), cin, cout, taps, dil, 1, 1)
        a = torch.where(x > 0, x, x * slope)                               # fp32(x * fp32(0.1)): the operand the device stages
        want_G, want_db = H.wgrad_reference(_masked(a), _masked(dy), taps, dil, 1, 0)
        bound_G, bound_db = H.wgrad_reference(_masked(a).abs(), _masked(dy).abs(), taps, dil, 1, 0)
        err = (G.double() - want_G).abs()
        print(f'wgrad lrelu ({taps}, {dil}) {cin}->{cout}: max err / bound {(err / (n_terms * EPS * bound_G)).max().item():.3f}')
        assert (err <= n_terms * EPS * bound_G).all(), (cin, cout)
        assert ((db.double() - want_db).abs() <= n_terms * EPS * bound_db).all(), (cin, cout)


def test_wgrad_of_conv_pre_reads_the_mel_through_its_strides():
    g = torch.Generator().manual_seed(80)
    for cout in (16, 128):
        mel, dy = _dyadic(g, B, 80, N), _dyadic(g, B, N, cout)              # (B, 80, T): element (b, n, c) at b 80 T + c T + n
        G, db = _wgrad(mel.to(DEV), (80 * N, 1, N), dy.to(DEV), 80, cout, 7, 1, 1, 0)
        _check_exact(mel.transpose(1, 2), dy, G, db, 7, 1, 1, cout)


@pytest.mark.parametrize('u', [2, 8])
def test_wgrad_of_a_transposed_conv_through_the_phase_view(u):
    g = torch.Generator().manual_seed(u)
    for cin, cout in WIDTHS:
        x, dy = _dyadic(g, B, N, cin), _dyadic(g, B, N * u, cout)
        G, db = _wgrad(x.to(DEV), (N * cin, cin, 1), dy.to(DEV), cin, cout, 3, 1, u, 0)
        _check_exact(x, dy, G, db, 3, 1, u, (cin, cout))
        a_dev = x.to(DEV)
        G1, db1 = _wgrad(a_dev, (N * cin, cin, 1), dy.to(DEV), cin, cout, 3, 1, u, 1)       # with the activation, as ups.i runs it
        a = torch.where(x > 0, x, x * torch.tensor(0.1))
        want_G, _ = H.wgrad_reference(_masked(a), _masked(dy, u), 3, 1, u, 0)
        bound_G, _ = H.wgrad_reference(_masked(a).abs(), _masked(dy, u).abs(), 3, 1, u, 0)
        assert ((G1.double() - want_G).abs() <= sum(ROWS) * EPS * bound_G).all(), (cin, cout)
        assert torch.equal(db1, db)


def test_wgrad_split_over_many_tiles_is_exact_and_reproducible():
    """Runs of several tiles (the position axis is cut into at most 682 runs here, whose partial sums a second launch adds in order;
    2 x 1094 tiles make runs of four): 16-wide operands, multiples of 1/2 in [-1, 1], so that the 82345-term sums stay exact."""
    g = torch.Generator().manual_seed(11)
    n, rows = 70000, (70000, 12345)
    x = torch.randint(-2, 3, (B, n, 16), generator=g).float() / 2
    dy = torch.randint(-2, 3, (B, n, 16), generator=g).float() / 2
    G, db = _wgrad(x.to(DEV), (n * 16, 16, 1), dy.to(DEV), 16, 16, 3, 1, 1, 0, n=n, rows=rows)
    want_G, want_db = H.wgrad_reference(_masked(x, 1, rows), _masked(dy, 1, rows), 3, 1, 1, 0)
    assert torch.equal(G.double(), want_G) and torch.equal(db.double(), want_db)
    G2, db2 = _wgrad(x.to(DEV), (n * 16, 16, 1), dy.to(DEV), 16, 16, 3, 1, 1, 0, n=n, rows=rows)
    assert torch.equal(G, G2) and torch.equal(db, db2)


@pytest.mark.parametrize('C', [16, 64])
def test_act_bwd_is_exact_on_dyadic_inputs(C):
    """dX = fp32( (acc ? dX : 0) + R + fp32(gscale * slope) * U ): one rounding (the device's fma), zero at and past the row's length."""
    g = torch.Generator().manual_seed(C)
    L, fr = lib(), _frames()
    x, u, r, old = (_dyadic(g, B, N, C) for _ in range(4))
    slope = torch.where(x > 0, torch.tensor(1.0), torch.tensor(0.1, dtype=torch.float32))
    for with_x, with_r, acc, gscale in ((1, 1, 0, 1.0), (1, 0, 0, 1.0), (0, 0, 0, 0.5), (1, 1, 1, 0.5), (1, 0, 1, 1.0)):
        s = (slope if with_x else torch.ones_like(x)) * torch.tensor(gscale, dtype=torch.float32)       # fp32 product, as on the device
        want = s.double() * u.double() + (r.double() if with_r else 0) + (old.double() if acc else 0)
        want = H._mask(want, list(ROWS), 1).float()
        xd, ud, rd, out = x.to(DEV), u.to(DEV), r.to(DEV), old.to(DEV).clone()
        L.dx_voc_act_bwd(xd.data_ptr() if with_x else None, ud.data_ptr(), rd.data_ptr() if with_r else None, out.data_ptr(), fr.data_ptr(), 1, B, N,
                         C, gscale, acc, _stream())
        assert torch.equal(out.cpu(), want), (with_x, with_r, acc, gscale)
    xd, ud, rd = x.to(DEV), u.to(DEV), r.to(DEV)                          # R may be dX: the residual chain runs in place
    L.dx_voc_act_bwd(xd.data_ptr(), ud.data_ptr(), rd.data_ptr(), rd.data_ptr(), fr.data_ptr(), 1, B, N, C, 1.0, 0, _stream())
    assert torch.equal(rd.cpu(), H._mask(slope.double() * u.double() + r.double(), list(ROWS), 1).float())


@pytest.mark.parametrize('C', [16, 32])
@pytest.mark.parametrize('n,rows', [(70, (70, 33)), (1100, (1100, 300))])       # one pass; several passes and two workgroups per row
def test_post_bwd_against_float64(C, n, rows):
    """y, dy, w, x multiples of 1/4: dz = dy (1 - y^2) and the seven-term sums of dz w are exact, so dX = fp32(slope * sum) and db
    must EQUAL float64; dw sums lrelu(x) dz, a = fp32(x * fp32(0.1)) not dyadic: within n_terms * 2^-24 * sum |a| |dz|."""
    g = torch.Generator().manual_seed(C + n)
    L = lib()
    x, w = _dyadic(g, B, n, C), _dyadic(g, 1, C, 7)
    y, dy = torch.randint(-4, 5, (B, n), generator=g).float() / 4, _dyadic(g, B, n)
    fr = torch.tensor(rows, dtype=torch.int32, device=DEV)
    nb = torch.zeros(1, dtype=torch.long)
    L.dx_voc_post_bwd_size(B, n, C, nb.data_ptr())
    ws = torch.full((int(nb) // 4,), float('nan'), device=DEV)
    xd, wd, yd, dyd = x.to(DEV), w.to(DEV), y.to(DEV), dy.to(DEV)
    dX, dW, db = torch.full((B, n, C), float('nan'), device=DEV), torch.full((1, C, 7), float('nan'), device=DEV), torch.full((1,), float('nan'), device=DEV)
    L.dx_voc_post_bwd(xd.data_ptr(), n * C, wd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), n, dX.data_ptr(), dW.data_ptr(), db.data_ptr(),
                      ws.data_ptr(), int(nb), fr.data_ptr(), 1, B, n, C, _stream())
    dz = H._mask(dy.double() * (1 - y.double() ** 2), list(rows), 1)
    xm = H._mask(x.double(), list(rows), 1)
    u = torch.nn.functional.conv1d(dz[:, None, :], w.double().flip(2).transpose(0, 1), padding=3).transpose(1, 2)
    slope = torch.where(x > 0, torch.tensor(1.0), torch.tensor(0.1, dtype=torch.float32)).double()
    assert torch.equal(dX.cpu(), H._mask(slope * u, list(rows), 1).float())
    assert torch.equal(db.cpu().double(), dz.sum().reshape(1))
    a = H._mask(torch.where(x > 0, x, x * torch.tensor(0.1)).double(), list(rows), 1)
    want, _ = H.wgrad_reference(a, dz[:, :, None], 7, 1, 1, 0)
    bound, _ = H.wgrad_reference(a.abs(), dz[:, :, None].abs(), 7, 1, 1, 0)
    assert ((dW.cpu().double() - want).abs() <= sum(rows) * EPS * bound).all()
