"""The upsampler / loss checks themselves, tested without a GPU (tests/upsample_loss_exact_helpers.py keeps
test_upsample_loss_exact_gpu.py honest):
(a) the restated LDS formulas reproduce the backward's switch of tile width at L = 416 / 417 and the two refusal lengths;
(b) the one-hot tier's claim holds in fp32 numpy: the weights are exactly {0, 1};
(c) plain fp32 torch (the oracle, for the upsampler's forward) passes every comparison on every case's inputs, every frame below an
    utterance's total compared: the bounds are attainable;
(d) every planted error fails its comparison, by a printed margin: a bound under which one passes would be too loose."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import upsample_loss_exact_helpers as ux

F32, F64 = torch.float32, torch.float64


def show(what, **figures):
    print(f'{what}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in figures.items()))


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
def test_restated_lds_formulas_give_the_switch_and_the_refusals():
    assert ux.bwd_tile(416) == 32 and ux.bwd_tile(417) == 16
    assert ux.first_over(lambda L: ux.bwd_smem(L, 32)) == 417
    assert ux.first_over(lambda L: ux.bwd_smem(L, 16)) == 849 and ux.bwd_tile(848) == 16 and ux.bwd_tile(849) is None
    assert ux.first_over(ux.fwd_smem) == 2120


# ---- duration scan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', ux.SCAN_LENGTHS)
def test_scan_restatement_and_its_lost_carry(L):
    d = ux.scan_inputs(L)
    mu, totals = ux.scan_ref(d)
    assert torch.equal(totals, d.sum(1)) and int(totals[1]) > 2 ** 24 and bool((d[0] == 0).any() or L == 1)
    want = d.double() / 2 + (torch.cumsum(d, 1) - d).double()                  # exact in float64: mu is its fp32 rounding, twice at most
    assert float(((mu.double() - want).abs() / want.abs().clamp_min(1)).max()) <= 2 * 2.0 ** -24
    small = d[0:1]
    assert torch.equal(ux.scan_ref(small)[0].double(), small.double() / 2 + (torch.cumsum(small, 1) - small).double())
    lost, _ = ux.scan_ref(d, lost_carry=True)
    if L > 64:
        wrong = int((~(lost.view(torch.int32) == mu.view(torch.int32))).sum())
        show(f'scan L={L}, carry lost at lane 64', elements_wrong=wrong)
        assert wrong > 0 and not ux.bits_equal(lost, mu)
    else:
        assert ux.bits_equal(lost, mu)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
def test_onehot_weights_are_exactly_zero_or_one_in_fp32_numpy():
    c = ux.onehot_case()
    mu, sg = c['mu'].numpy(), c['sigma'].numpy()
    assert mu.dtype == np.float32 and sg.dtype == np.float32
    t = (np.arange(c['T'], dtype=np.float32) + np.float32(0.5))[None, None, :]
    d = t - mu[:, :, None]
    with np.errstate(under='ignore'):
        p = np.exp(-(d * d) / (np.float32(2) * (sg * sg))[:, :, None] - np.log(sg)[:, :, None] - np.float32(ux.LOG_SQRT_2PI))
    assert p.dtype == np.float32
    p = p * ux.valid_mask(c['lens'], c['L']).numpy()[:, :, None]
    den = p.sum(1, dtype=np.float32) + np.float32(1e-20)
    w = p / den[:, None, :]
    want, xup, dxs = ux.onehot_expected(c)
    assert np.array_equal(w, want.numpy()) and set(np.unique(w)) == {0.0, 1.0}
    assert float(p.max()) > 398 and float(np.float32(1e-20)) < np.spacing(np.float32(398))     # 1e-20 is below the numerator's ulp
    assert 0.2 < float(want.sum()) / float(c['totals'].sum()) < 0.8                          # centre frames and empty frames both occur
    per_frame = want.sum(1)
    assert float(per_frame.max()) == 1.0 and bool((per_frame[0, :int(c['totals'][0])] == 0).any())
    centres = want[0].sum(0).nonzero()[:, 0]
    assert len({int(t) // 16 for t in centres}) >= 3                                            # centre frames in several 16-frame tiles
    # and the float64 restatement agrees with the construction
    _, _, w64 = ux.weights_ref(c['mu'], c['sigma'], c['lens'], c['T'])
    assert torch.equal(w64.float(), want)
    dxs64, ds64 = ux.bwd_ref(c, want)
    assert torch.equal(dxs64.float(), dxs) and float(ds64.abs().max()) == 0.0


# ---- (c), upsampler -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cases():
    return {n: ux.upsample_case(n) for n in ux.ROUNDED_CASES}


@pytest.fixture(scope='module')
def fp32_forward(cases):
    out = {}
    for n, c in cases.items():
        _, _, w = ux.weights_ref(c['mu'], c['sigma'], c['lens'], c['T'], F32)
        out[n] = (w, ux.xup_ref(w, c['xs'], F32))
    return out


def test_case_shapes_reach_their_edges(cases):
    a, b, d = cases['a'], cases['b'], cases['d']
    assert a['T'] % 16 != 0 and int(a['totals'][3]) == 0 and a['lens'][3] == 1
    assert b['T'] % 32 == 1 and int(b['totals'][1]) == 96 and float(b['dxup'][1, 96:].abs().max()) == 0 and float(b['base_dsigma'].abs().max()) > 0
    assert ux.bwd_tile(cases['c416']['L']) == 32 and ux.bwd_tile(cases['c417']['L']) == 16
    assert d['L'] == 32 and max(d['lens']) <= 20 and d['T'] == 128 and int(d['totals'].max()) <= 90
    for c in cases.values():
        v = ux.valid_mask(c['lens'], c['L'])
        assert float(c['sigma'][v].min()) >= 0.5 and float(c['sigma'][v].max()) <= 4 and int(c['dur_int'].max()) <= 6


@pytest.mark.parametrize('name', ux.ROUNDED_CASES)
def test_fp32_torch_passes_the_forward_bounds(cases, fp32_forward, name):
    c = cases[name]
    w, xup = fp32_forward[name]
    r = ux.check_forward(c, w, xup)
    show(f'forward {name}, fp32 torch', **r)
    assert r['weights'] <= 1 and r['xup'] <= 1


@pytest.mark.parametrize('name', ['a', 'b', 'c417'])
def test_the_oracle_passes_the_forward_bounds(cases, name):
    """oracle.gaussian_upsampling in fp32, its sigma rebuilt by the same torch calls (same bits), against the float64 restatement"""
    from oracle import daft_exprt_oracle as oracle
    c = dict(cases[name])
    B, L = c['B'], c['L']
    p = ux.prep_inputs(B, L, c['lens'], 1.0, 0.05, seed=9)
    gp = 'gaussian_upsampling.'
    sd = {gp + 'duration_projection.conv.weight': p['wd'], gp + 'duration_projection.conv.bias': p['bd'],
          gp + 'energy_projection.conv.weight': p['we'], gp + 'energy_projection.conv.bias': p['be'],
          gp + 'pitch_projection.conv.weight': p['wp'], gp + 'pitch_projection.conv.bias': p['bp'],
          gp + 'projection.0.linear_layer.weight': p['wr'][None, :], gp + 'projection.0.linear_layer.bias': p['br']}
    lens = torch.tensor(c['lens'])
    xup, w = oracle.gaussian_upsampling(sd, p['enc'], p['dur'], c['dur_int'], p['energy'], p['pitch'], lens)
    x = p['enc'] + oracle.conv_cl(sd, gp + 'energy_projection', p['energy'][:, :, None]) + oracle.conv_cl(sd, gp + 'pitch_projection', p['pitch'][:, :, None])
    rng = F.softplus(oracle.linear(sd, gp + 'projection.0', x + oracle.conv_cl(sd, gp + 'duration_projection', p['dur'][:, :, None]))).squeeze(2)
    c['xs'], c['sigma'] = x, rng.masked_fill(~ux.valid_mask(c['lens'], L), 1.0).clamp(min=1e-3)
    assert w.shape == (B, L, c['T']) and xup.shape == (B, c['T'], ux.D)
    r = ux.check_forward(c, w, xup)
    show(f'forward {name}, oracle', **r)
    assert r['weights'] <= 1 and r['xup'] <= 1


@pytest.mark.parametrize('name', ux.ROUNDED_CASES)
def test_fp32_torch_passes_the_backward_bounds(cases, fp32_forward, name):
    c = cases[name]
    w = fp32_forward[name][0]
    dxs, dsigma = ux.bwd_ref(c, w, F32)
    r = ux.check_backward(c, w, c['base_dxs'] + dxs, c['base_dsigma'] + dsigma)
    show(f'backward {name}, fp32 torch', **r)
    assert r['dxs'] <= 1 and r['dsigma'] <= 1


# ---- (d), upsampler -----------------------------------------------------------------------------------------------------------------
def _busy_symbol(c, b=0):
    """a symbol of row b with a duration of at least 2, its centre frame and that frame's 16-frame tile"""
    l = next(l for l in range(5, c['lens'][b]) if int(c['dur_int'][b, l]) >= 2)
    t = int(float(c['mu'][b, l]))
    return l, t, (t // 16) * 16


@pytest.mark.parametrize('name', ['b', 'c417'])
def test_planted_forward_errors_fail(cases, name):
    c = cases[name]
    l, t, t0 = _busy_symbol(c)
    _, _, w = ux.weights_ref(c['mu'], c['sigma'], c['lens'], c['T'], F32)
    # one xs element changed by 2^-10 relative
    ch = int(c['xs'][0, l].abs().argmax())
    xs = c['xs'].clone()
    xs[0, l, ch] *= 1 + 2.0 ** -10
    r = ux.check_forward(c, w, ux.xup_ref(w, xs, F32))
    show(f'{name}: xs[0, {l}, {ch}] off by 2^-10', xup=r['xup'])
    assert r['weights'] <= 1 < r['xup']
    # one symbol row dropped from one frame tile
    wd = w.clone()
    wd[0, l, t0:t0 + 16] = 0
    r = ux.check_forward(c, w, ux.xup_ref(wd, c['xs'], F32))
    show(f'{name}: symbol {l} dropped from the tile at {t0}', xup=r['xup'])
    assert r['xup'] > 1
    # one sigma changed by 1e-3 relative
    sg = c['sigma'].clone()
    sg[0, l] *= 1 + 1e-3
    _, _, ws = ux.weights_ref(c['mu'], sg, c['lens'], c['T'], F32)
    r = ux.check_forward(c, ws, ux.xup_ref(ws, c['xs'], F32))
    show(f'{name}: sigma[0, {l}] off by 1e-3', weights=r['weights'], xup=r['xup'])
    assert r['weights'] > 1


@pytest.mark.parametrize('name', ['b', 'c417'])
def test_planted_backward_errors_fail(cases, fp32_forward, name):
    c = cases[name]
    l, t, t0 = _busy_symbol(c)
    w = fp32_forward[name][0]
    TT = ux.bwd_tile(c['L'])
    t0 = (t // TT) * TT
    base = lambda dxs, ds: (c['base_dxs'] + dxs, c['base_dsigma'] + ds)
    # one frame's gradient dropped
    g = c['dxup'].clone()
    g[0, t] = 0
    r = ux.check_backward(c, w, *base(*ux.bwd_ref(c, w, F32, dxup=g)))
    show(f'{name}: gradient of frame {t} dropped', dxs=r['dxs'], dsigma=r['dsigma'])
    assert r['dxs'] > 1 and r['dsigma'] > 1
    # one symbol row dropped from one frame tile (its weights read as zero there)
    wd = w.clone()
    wd[0, l, t0:t0 + TT] = 0
    r = ux.check_backward(c, w, *base(*ux.bwd_ref(c, wd, F32)))
    show(f'{name}: symbol {l} dropped from the tile at {t0}', dxs=r['dxs'], dsigma=r['dsigma'])
    assert r['dxs'] > 1 and r['dsigma'] > 1
    # one sigma changed by 1e-3 relative
    sg = c['sigma'].clone()
    sg[0, l] *= 1 + 1e-3
    r = ux.check_backward(c, w, *base(*ux.bwd_ref(c, w, F32, sigma=sg)))
    show(f'{name}: sigma[0, {l}] off by 1e-3', dxs=r['dxs'], dsigma=r['dsigma'])
    assert r['dxs'] <= 1 < r['dsigma']
    # a skipped tile that was not empty: the frame tile's whole gradient missing
    g = c['dxup'].clone()
    g[0, t0:t0 + TT] = 0
    r = ux.check_backward(c, w, *base(*ux.bwd_ref(c, w, F32, dxup=g)))
    assert r['dxs'] > 1 and r['dsigma'] > 1
    # the base overwritten instead of accumulated onto
    if float(c['base_dxs'].abs().max()) > 0:
        r = ux.check_backward(c, w, *ux.bwd_ref(c, w, F32))
        assert r['dxs'] > 1 and r['dsigma'] > 1


# ---- prep and symbol backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ux.PREP_CASES))
def test_fp32_torch_passes_the_prep_bounds_and_the_cases_reach_their_regimes(name):
    p = ux.prep_case(name)
    B, L = p['enc'].shape[:2]
    xs = ux.prep_xs(p, F32)
    z = ux.prep_z(p, xs, F32)
    sg = ux.prep_sigma(z, p['lens'], F32)
    v = ux.valid_mask(p['lens'], L)
    r_xs, _ = ux.worst_ratio(xs, ux.prep_xs(p), ux.prep_xs_bound(p))
    r_z, _ = ux.worst_ratio(z, ux.prep_z(p, xs), ux.prep_z_bound(p, xs))
    s64 = ux.prep_sigma(z, p['lens'])
    r_s, _ = ux.worst_ratio(sg, s64, ux.prep_sigma_bound(s64))
    big, tiny = (z > 20)[v], (s64 <= ux.SIGMA_MIN)[v]
    show(f'prep {name}, fp32 torch', xs=r_xs, z=r_z, sigma=r_s, z_above_20=float(big.float().mean()), clamped=float(tiny.float().mean()))
    assert r_xs <= 1 and r_z <= 1 and r_s <= 1
    if name != 'small':
        assert B * L == 16385 and (B * L + 3) // 4 > ux.PREP_MAX_BLOCKS and (B * L) % 4 != 0
    if name == 'large_z':
        assert bool(big.all())
    if name == 'tiny_softplus':
        assert bool(tiny.all())
    if name == 'straddle':
        assert 0.02 < float(big.float().mean()) < 0.9 and 0.02 < float(tiny.float().mean()) < 0.9
    assert bool((s64[~v] == 1).all())
    # a wrong tap: the energy stream read one symbol late
    bad = dict(p, energy=torch.roll(p['energy'], 1, 1))
    assert ux.worst_ratio(ux.prep_xs(bad, F32), ux.prep_xs(p), ux.prep_xs_bound(p))[0] > 1


def test_fp32_torch_passes_the_symbol_backward_bounds_and_planted_gates_fail():
    p = ux.sym_bwd_inputs()
    rows = p['B'] * p['L']
    assert rows == 1027 and (rows + 3) // 4 > ux.SYM_BWD_BLOCKS and rows % 4 != 0
    dz64, cmp = ux.sym_dz(p)
    v = ux.valid_mask(p['lens'], p['L'])
    excluded = int((~cmp).sum())
    assert 0 < excluded <= ux.MAX_EXCLUDED * int(v.sum())
    z = p['z'].double()
    for lo, hi in ((ux.Z_GATE, 1e-4), (ux.SOFTPLUS_T, 1e-3)):                     # compared values close on either side of both thresholds
        assert bool((cmp & v & (z > lo) & (z < lo + hi)).any()) and bool((cmp & v & (z < lo) & (z > lo - hi)).any())
    dz = ux.sym_dz(p, F32)[0]
    r_dz, _ = ux.worst_ratio(dz, dz64, 8 * ux.U * dz64.abs(), cmp)
    out, dwr, dbr = ux.sym_rest(p, dz, F32)
    ro, rw, rb = (ux.worst_ratio(g, r, b)[0] for g, r, b in zip((out, dwr, dbr), ux.sym_rest(p, dz), ux.sym_bounds(p, dz)))
    show('symbol backward, fp32 torch', dz=r_dz, dxs_out=ro, dwr=rw, dbr=rb, excluded=excluded)
    assert max(r_dz, ro, rw, rb) <= 1
    # the clamp's gate ignored; sigmoid used beyond 20 is the same number in fp32, so the other planted error is the length mask
    ungated = torch.where(v, p['dsigma'] * torch.sigmoid(p['z']), torch.zeros(1))
    assert ux.worst_ratio(ungated, dz64, 8 * ux.U * dz64.abs(), cmp)[0] > 1
    unmasked = torch.where(ux.softplus(p['z'].double()) >= ux.SIGMA_MIN, (torch.randn(p['B'], p['L']) * torch.sigmoid(p['z'])).double(), torch.zeros(1, dtype=F64))
    assert ux.worst_ratio(unmasked * ~v + dz64 * v, dz64, 8 * ux.U * dz64.abs(), cmp)[0] > 1
    # one row missing from dwr / dbr
    dz_drop = dz.clone()
    dz_drop[3, 7] = 0
    _, dwr_d, dbr_d = ux.sym_rest(p, dz_drop, F32)
    b = ux.sym_bounds(p, dz)
    margins = ux.worst_ratio(dwr_d, ux.sym_rest(p, dz)[1], b[1])[0], ux.worst_ratio(dbr_d, ux.sym_rest(p, dz)[2], b[2])[0]
    show('symbol backward, one row missing from the parameter gradients', dwr=margins[0], dbr=margins[1])
    assert min(margins) > 1


# ---- loss -----------------------------------------------------------------------------------------------------------------------------
def _poison(c, ep, et):
    if c['rows_exist'] is None:
        return ep, et
    ep, et = ep.clone(), et.clone()
    for b, r in enumerate(c['rows_exist']):
        ep[b, r:] = float('nan')
        et[b, r:] = float('nan')
    return ep, et


@pytest.mark.parametrize('name', list(ux.LOSS_CASES))
def test_fp32_torch_passes_the_loss_bounds(name):
    c = ux.loss_case(name)
    ref = ux.mel_stats_ref(c['mp'], c['mt'])
    got = ux.mel_stats_ref(c['mp'], c['mt'], F32)
    bounds = ux.mel_stats_bounds(ref, c['M'], c['T'])
    r = {k: ux.worst_ratio(got[k], ref[k], bounds[k])[0] for k in ref}
    ep, et = _poison(c, got['ep'], got['et'])
    des, esum, _ = ux.energy_ref(ep, et, c['lens'], c['rows_exist'], F32)
    des64, esum64, _ = ux.energy_ref(ep, et, c['lens'], c['rows_exist'])
    b_des, b_esum = ux.energy_bounds(ep, et, c['lens'], c['rows_exist'])
    r['des'], r['esum'] = ux.worst_ratio(des, des64, b_des)[0], ux.worst_ratio(esum, esum64, b_esum)[0]
    dmel64, b_dmel = ux.mel_grad_ref(c, got['ep'], des)
    r['dmel'] = ux.worst_ratio(ux.mel_grad_ref(c, got['ep'], des, F32)[0], dmel64, b_dmel)[0]
    show(f'loss {name}, fp32 torch', **r)
    assert max(r.values()) <= 1
    d = c['mp'] - c['mt']
    v = ux.valid_mask(c['lens'], c['T'])[:, None, :].expand_as(d)
    assert float(d[~v].abs().max() if bool((~v).any()) else 0) == 0 and float(c['mp'][~v].abs().max() if bool((~v).any()) else 0) == 0
    if d[v].numel() > 1000:
        assert 0.003 < float((d[v] == 0).float().mean()) < 0.03                # the sign-0 cells


def test_loss_restatement_is_the_torch_loss_and_its_autograd():
    """the float64 restatement against loss.py's formulas written with torch (avg_pool1d, norm, autograd), as test_loss_kernels does"""
    c = ux.loss_case('edge64')
    B, M, T = c['B'], c['M'], c['T']
    lens = torch.tensor(c['lens'])
    v = ux.valid_mask(c['lens'], T)
    mp = c['mp'].double().requires_grad_(True)
    mt = c['mt'].double()
    denom = M * lens.double()
    l1 = ((mp - mt).abs().sum((1, 2)) / denom).mean()
    l2 = (((mp - mt) ** 2).sum((1, 2)) / denom).mean()
    pe = F.avg_pool1d(torch.norm(torch.exp(mp), dim=1)[:, None], 5, 1, 2)[:, 0]
    te = F.avg_pool1d(torch.norm(torch.exp(mt), dim=1)[:, None], 5, 1, 2)[:, 0]
    en = (((pe - te) ** 2) * v).sum() / lens.sum()
    (l1 + l2 + 0.05 * en).backward()
    ref = ux.mel_stats_ref(c['mp'], c['mt'])
    des, esum, _ = ux.energy_ref(ref['ep'], ref['et'], c['lens'], None)
    dmel, _ = ux.mel_grad_ref(dict(c, c_l1=1.0 / (M * B), c_l2=1.0 / (M * B), c_e=0.05 / float(lens.sum())), ref['ep'], des)
    l1, en = float(l1.detach()), float(en.detach())
    assert abs(float((ref['l1'] / denom).mean()) - l1) <= 1e-12 * l1 and abs(float(esum / lens.sum()) - en) <= 1e-12 * en
    assert float((dmel - mp.grad).abs().max()) <= 1e-6 * float(mp.grad.abs().max())     # c_l1 .. c_e pass through fp32


def test_planted_loss_errors_fail():
    # one pooling neighbour dropped at a block edge: frame 256 from the window of frame 255 (energy_diff), frame 64 from that of 63 (mel_grad)
    c = ux.loss_case('edge256')
    ref = ux.mel_stats_ref(c['mp'], c['mt'], F32)
    des64, esum64, _ = ux.energy_ref(ref['ep'], ref['et'], c['lens'], None)
    b_des, b_esum = ux.energy_bounds(ref['ep'], ref['et'], c['lens'], None)
    des, esum, _ = ux.energy_ref(ref['ep'], ref['et'], c['lens'], None, F32, drop=(0, 255, 256))
    r, at = ux.worst_ratio(des, des64, b_des)
    show('des: frame 256 missing from the window of frame 255', margin=r, at=at, esum=ux.worst_ratio(esum, esum64, b_esum)[0])
    assert r > 1 and at == (0, 255)
    des = ux.energy_ref(ref['ep'], ref['et'], c['lens'], None, F32)[0]
    dmel64, b_dmel = ux.mel_grad_ref(c, ref['ep'], des)
    r, at = ux.worst_ratio(ux.mel_grad_ref(c, ref['ep'], des, F32, drop=(0, 63, 64))[0], dmel64, b_dmel)
    show('dmel: frame 64 missing from the window of frame 63', margin=r, at=at)
    assert r > 1 and at[0] == 0 and at[2] == 63
    # rows_exist ignored: with the poison, and with the finite energies the model's buffers hold there
    c = ux.loss_case('rows_exist')
    ref = ux.mel_stats_ref(c['mp'], c['mt'], F32)
    b_des, _ = ux.energy_bounds(ref['ep'], ref['et'], c['lens'], c['rows_exist'])
    des64 = ux.energy_ref(ref['ep'], ref['et'], c['lens'], c['rows_exist'])[0]
    for ep, et in (_poison(c, ref['ep'], ref['et']), (ref['ep'], ref['et'] * 1.25)):
        r, at = ux.worst_ratio(ux.energy_ref(ep, et, c['lens'], c['rows_exist'], F32, ignore_rows_exist=True)[0], des64, b_des)
        show('des: rows_exist ignored', margin=r, at=at)
        assert r > 1 and at[1] in (128, 129)                                  # row 0: length 130 = rows_exist
    # a sign that treats 0 as positive; a sum that loses one 64-frame block
    c = ux.loss_case('edge64')
    ref = ux.mel_stats_ref(c['mp'], c['mt'])
    b = ux.mel_stats_bounds(ref, c['M'], c['T'])
    lost = ux.mel_stats_ref(c['mp'][:, :, :64], c['mt'][:, :, :64], F32)
    assert ux.worst_ratio(lost['l1'], ref['l1'], b['l1'])[0] > 1 and ux.worst_ratio(lost['l2'], ref['l2'], b['l2'])[0] > 1
    des = ux.energy_ref(ref['ep'], ref['et'], c['lens'], None, F32)[0]
    dmel64, b_dmel = ux.mel_grad_ref(c, ref['ep'], des)
    d = c['mp'] - c['mt']
    v = ux.valid_mask(c['lens'], c['T'])[:, None, :]
    wrong = dmel64 + ((d == 0) & v) * (c['c_l1'] / torch.tensor(c['lens']).double()[:, None, None])
    assert ux.worst_ratio(wrong, dmel64, b_dmel)[0] > 1


@pytest.mark.parametrize('name', list(ux.PITCH_CASES))
def test_fp32_torch_passes_the_pitch_bounds(name):
    B, T, lens = ux.PITCH_CASES[name]
    c = ux.pitch_inputs(B, T, lens)
    s64, n64, b = ux.pitch_ref(c)
    s32, n32, _ = ux.pitch_ref(c, F32)
    g64, bg = ux.pitch_grad_ref(c, n64, 0.15)
    r = ux.worst_ratio(s32.reshape(1), s64.reshape(1), b)[0], ux.worst_ratio(ux.pitch_grad_ref(c, n32, 0.15, F32)[0], g64, bg)[0]
    show(f'pitch {name}, fp32 torch', sum=r[0], grad=r[1])
    assert n32 == n64 and max(r) <= 1
    if T > 1:
        m = ux.valid_mask(lens, T)
        assert bool(((c['gt'] == 0) & m).any()) and bool(((c['gt'] != 0) & m).any())
        lost = ux.pitch_ref(dict(c, pp=c['pp'][:, :256], gt=c['gt'][:, :256], T=256, lens=[256, 256, 100]), F32)[0]      # the second block lost
        assert ux.worst_ratio(lost.reshape(1), s64.reshape(1), b)[0] > 1
    u = ux.pitch_inputs(B, T, lens, all_unvoiced=True)
    assert ux.pitch_ref(u)[:2] == (0.0, 0.0) and float(ux.pitch_grad_ref(u, 0.0, 0.15)[0].abs().max()) == 0


@pytest.mark.parametrize('B', [3, 300])
@pytest.mark.parametrize('off', ux.FINALIZE_SWITCHES)
def test_fp32_torch_passes_the_finalize_bounds(B, off):
    f = ux.finalize_inputs(B, [1 + (5 * b) % 7 for b in range(B)])
    ref, got = ux.finalize_ref(f, off), ux.finalize_ref(f, off, F32)
    r = {k: ux.worst_ratio(got[k][0], ref[k][0], ref[k][1])[0] for k in ref}
    show(f'finalize B={B}, {off} off, fp32 torch', **r)
    assert max(r.values()) <= 1 and set(ref) == {'terms', 'total'} | ({'d_spk'} if off != 'ce' else set()) | ({'d_pm'} if off != 'pm' else set())
    idx = {'ce': (0, 1), 'pm': (2,), 'esum': (5,), 'psum': (6,)}.get(off, ())
    assert all(float(ref['terms'][0][i]) == 0 for i in idx) and int((ref['terms'][0] != 0).sum()) == 7 - len(idx)
    # a term left out of the total
    t = ref['terms'][0]
    assert ux.worst_ratio(ref['total'][0] - t[3], ref['total'][0], ref['total'][1])[0] > 1


@pytest.mark.parametrize('B', [5, 257])
def test_fp32_torch_passes_the_cross_entropy_bounds(B):
    logits, target = ux.cross_entropy_inputs(B)
    loss, dl, b_loss, b_dl = ux.cross_entropy_ref(logits, target)
    l32 = logits.clone().requires_grad_(True)
    t_loss = F.cross_entropy(l32, target)
    t_loss.backward()
    r = ux.worst_ratio(t_loss.reshape(1), loss, b_loss)[0], ux.worst_ratio(l32.grad, dl, b_dl)[0]
    show(f'cross entropy B={B}, fp32 torch', loss=r[0], dlogits=r[1])
    assert max(r) <= 1
    assert ux.worst_ratio(l32.grad * B / 256 if B > 256 else l32.grad * (1 + 2.0 ** -18), dl, b_dl)[0] > 1
