"""The Gaussian upsampler (csrc/dx_upsample.hip), the loss kernels (csrc/dx_loss.hip) and dx_cross_entropy, element by element against
float64 (tests/upsample_loss_exact_helpers.py states the restatements, the inputs and the a-priori bounds;
tests/test_upsample_loss_exact_cpu.py tests that statement and shows that plain fp32 torch attains every bound).  The C entries are
called directly, on buffers of the test's own: outputs pre-filled with a sentinel, accumulated outputs with a dyadic base.  Later
stages are handed the device output of the stage before, after that output has been checked, and so is their restatement.

The bounds were fixed before anything was measured and are not tuned to the figures below.  Both tile widths of dx_upsample_bwd run:
L = 416 is the last length on 32-frame tiles, L = 417 the first on 16-frame tiles (asserted from the restated LDS formula).

Measured on the MI355X: the worst ratio of |device - float64| to the bound, per output, over the cases of each group ("The
upsampler and the loss against float64"; the outputs summed through atomics move in the last digit from run to run):
  duration scan, 5 lengths        mu and totals bitwise (totals past 2^24, the carry across 64-lane chunks)
  one-hot tier                    weights, x_up, dxs, dsigma bitwise
  rounded tier a, b, d            weights 0.24   x_up 0.073   dxs 0.087   dsigma 0.0010     (32-frame tiles)
  rounded tier L = 416            weights 0.16   x_up 0.0099  dxs 0.096   dsigma 0.0013     (32-frame tiles)
  rounded tier L = 417            weights 0.16   x_up 0.0092  dxs 0.085   dsigma 0.00079    (16-frame tiles)
  prep, 16 385 rows x 3, 21 rows  xs 0.31   z 0.052   sigma 0.23 (0 where every z > 20 or every softplus is clamped: exact)
  symbol backward, 1027 rows      dz 0.24   dxs_out 0.33   dwr 0.0052   dbr 0.00076   (3 rows within 4 ulp of the gate left out)
  mel / energy, 6 shapes          ep 0.16   et 0.14   l1sum 0.064   l2sum 0.074   des 0.19   esum 0.016   dmel 0.39
  pitch, 2 shapes x ld 1, 4       sum 0.030   gradient 0.33   count exact
  finalize, B = 3, 300 x 5        terms 0.36   total 0.047   d_spk 0.32   d_pm 0.096
  cross entropy, B = 5, 257       loss 0.019   dlogits 0.46
The element-wise outputs sit at 0.2 - 0.5 of their bounds, as plain fp32 torch does on the CPU; the sums sit far lower because a
worst-case summation bound grows with n and a real sum's error with its root.  dsigma's bound is the loosest: its magnitude sum is the
fully expanded one.  It still separates the planted errors (one sigma off by 1e-3: 1.8 - 2.2 x the bound; a dropped frame or symbol row:
about 300 x).  The three _dyn entries equal their static twins bit for bit at scales 2^-3 and 2^15 (tests/test_loss_scaler_gpu.py
asserts that through the whole loss, not per entry, so none is skipped here).  No kernel change was needed.
"""
import pytest
import torch

from tests import upsample_loss_exact_helpers as ux

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = -12345.5
D = ux.D


@pytest.fixture(scope='module')
def lib():
    from ubisoft_laforge_daft_exprt_amd import _lib
    return _lib.lib()


def P(t):
    return None if t is None else t.data_ptr()


def S():
    return torch.cuda.current_stream().cuda_stream


_ALIVE = []       # a launch gets raw pointers: every device copy made for one stays referenced until its test ends, so that no two of
                  # them share an address (a temporary's block goes back to the caching allocator at once and is handed out again)


@pytest.fixture(autouse=True)
def _keep_device_copies_alive():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def dev(t):
    _ALIVE.append(t.to(DEV).contiguous())
    return _ALIVE[-1]


def i32(vals):
    return None if vals is None else dev(torch.tensor(list(vals), dtype=torch.int32))


def filled(*shape, value=SENTINEL):
    return torch.full(shape, value, dtype=torch.float32, device=DEV)


def show(what, **figures):
    print(f'{what}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}' for k, v in figures.items()))


# ---- duration scan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', ux.SCAN_LENGTHS)
def test_duration_scan_is_bitwise(lib, L):
    d = ux.scan_inputs(L)
    mu, totals = filled(3, L), torch.full((3,), -7, dtype=torch.long, device=DEV)
    lib.dx_duration_scan(P(dev(d)), P(mu), P(totals), 3, L, S())
    torch.cuda.synchronize()
    want_mu, want_totals = ux.scan_ref(d)
    assert torch.equal(totals.cpu(), d.sum(1)) and torch.equal(totals.cpu(), want_totals) and int(totals[1]) > 2 ** 24
    assert ux.bits_equal(mu, want_mu), f'mu differs at {(mu.cpu() != want_mu).nonzero()[:4].tolist()}'


# ---- upsampler: launches ----------------------------------------------------------------------------------------------------------------
def run_fwd(lib, c):
    B, L, T = c['B'], c['L'], c['T']
    w, xup = filled(B, L, T), filled(B, T, D)
    lib.dx_upsample_fwd(P(dev(c['xs'])), P(dev(c['mu'])), P(dev(c['sigma'])), P(i32(c['lens'])), P(w), P(xup), B, L, T, D, S())
    torch.cuda.synchronize()
    return w, xup


def run_bwd(lib, c, w):
    B, L, T = c['B'], c['L'], c['T']
    dxs, dsigma = dev(c['base_dxs']).clone(), dev(c['base_dsigma']).clone()
    lib.dx_upsample_bwd(P(dev(c['dxup'])), P(dev(c['xs'])), P(dev(c['mu'])), P(dev(c['sigma'])), P(w), P(i32(c['lens'])), P(dxs), P(dsigma),
                        B, L, T, D, S())
    torch.cuda.synchronize()
    return dxs, dsigma


def test_onehot_tier_is_bitwise(lib):
    """sigma = 1e-3: every weight exactly 1 at the centre frame of an odd-duration symbol and 0 elsewhere, so x_up, dxs and dsigma are
    exact in any order: the MFMA operand layouts and the scatter, with no tolerance"""
    c = ux.onehot_case()
    want_w, want_xup, want_dxs = ux.onehot_expected(c)
    w, xup = run_fwd(lib, c)
    assert torch.equal(w.cpu(), want_w), f'{int((w.cpu() != want_w).sum())} weights are not the one-hot pattern'
    assert torch.equal(xup.cpu(), want_xup), f'x_up differs at {(xup.cpu() != want_xup).nonzero()[:4].tolist()}'
    centres = want_w.sum(1) > 0
    assert float(xup.cpu()[~centres].abs().max()) == 0 and len({int(t) // 16 for t in centres[0].nonzero()[:, 0]}) >= 3
    dxs, dsigma = run_bwd(lib, c, w)
    assert float(dsigma.abs().max()) == 0, 'dsigma is not exactly zero'
    assert torch.equal(dxs.cpu(), want_dxs), f'dxs differs at {(dxs.cpu() != want_dxs).nonzero()[:4].tolist()}'
    odd = (c['dur_int'] % 2 == 1) & ux.valid_mask(c['lens'], c['L'])
    assert float(dxs.cpu()[~odd].abs().max()) == 0 and bool((c['dur_int'][ux.valid_mask(c['lens'], c['L'])] == 0).any())


@pytest.mark.parametrize('name', ux.ROUNDED_CASES)
def test_rounded_tier_forward_and_backward(lib, name):
    c = ux.upsample_case(name)
    L, T = c['L'], c['T']
    v = ux.valid_mask(c['lens'], L)
    if name.startswith('c'):
        assert ux.bwd_tile(416) == 32 and ux.bwd_tile(417) == 16 and ux.bwd_tile(L) == (32 if name == 'c416' else 16)
    w, xup = run_fwd(lib, c)
    r = ux.check_forward(c, w, xup)
    show(f'forward {name}', **r)
    assert r['weights'] <= 1, f"weights: {r['weights']:.3g} x the bound at (b, l, t) = {r['weights_at']}"
    assert r['xup'] <= 1, f"x_up: {r['xup']:.3g} x the bound at (b, t, c) = {r['xup_at']}"
    assert float(w.cpu()[~v].abs().max() if bool((~v).any()) else 0) == 0, 'a weight of a symbol at or past the length is not exactly zero'
    dxs, dsigma = run_bwd(lib, c, w)
    r = ux.check_backward(c, w, dxs, dsigma)
    show(f'backward {name} ({ux.bwd_tile(L)}-frame tiles)', **r)
    assert r['dxs'] <= 1, f"dxs: {r['dxs']:.3g} x the bound at (b, l, c) = {r['dxs_at']}"
    assert r['dsigma'] <= 1, f"dsigma: {r['dsigma']:.3g} x the bound at (b, l) = {r['dsigma_at']}"
    if bool((~v).any()):                                  # rows at or past the length keep their bits
        assert ux.bits_equal(dxs.cpu()[~v], c['base_dxs'][~v]) and ux.bits_equal(dsigma.cpu()[~v], c['base_dsigma'][~v])


def test_upsampler_refuses_lengths_beyond_its_lds(lib):
    from ubisoft_laforge_daft_exprt_amd._lib import DxError
    Lb, Lf = ux.first_over(lambda L: ux.bwd_smem(L, 16)), ux.first_over(ux.fwd_smem)
    assert (Lb, Lf) == (849, 2120)
    T = 16
    for L, which in ((Lb, 'bwd'), (Lf, 'fwd')):
        xs, mu, sg, lens = filled(1, L, D, value=0.5), filled(1, L, value=3.0), filled(1, L, value=1.0), i32([L])
        if which == 'fwd':
            out = [filled(1, L, T), filled(1, T, D)]
            with pytest.raises(DxError):
                lib.dx_upsample_fwd(P(xs), P(mu), P(sg), P(lens), P(out[0]), P(out[1]), 1, L, T, D, S())
        else:
            out = [filled(1, L, D), filled(1, L)]
            w, g = filled(1, L, T, value=0.25), filled(1, T, D, value=1.0)
            with pytest.raises(DxError):
                lib.dx_upsample_bwd(P(g), P(xs), P(mu), P(sg), P(w), P(lens), P(out[0]), P(out[1]), 1, L, T, D, S())
        torch.cuda.synchronize()
        assert all(bool((o == SENTINEL).all()) for o in out), f'dx_upsample_{which} wrote something at L = {L}'


# ---- prep and symbol backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(ux.PREP_CASES))
def test_prep_elementwise(lib, name):
    p = ux.prep_case(name)
    B, L = p['enc'].shape[:2]
    xs, z, sg = filled(B, L, D), filled(B, L), filled(B, L)
    lib.dx_upsample_prep(*(P(dev(p[k])) for k in ('enc', 'dur', 'energy', 'pitch', 'wd', 'bd', 'we', 'be', 'wp', 'bp', 'wr', 'br')),
                         P(i32(p['lens'])), P(xs), P(z), P(sg), B, L, D, S())
    torch.cuda.synchronize()
    v = ux.valid_mask(p['lens'], L)
    r_xs, at_xs = ux.worst_ratio(xs, ux.prep_xs(p), ux.prep_xs_bound(p))
    assert r_xs <= 1, f'xs: {r_xs:.3g} x the bound at {at_xs}'
    r_z, at_z = ux.worst_ratio(z, ux.prep_z(p, xs), ux.prep_z_bound(p, xs))
    assert r_z <= 1, f'z: {r_z:.3g} x the bound at {at_z}'
    s64 = ux.prep_sigma(z, p['lens'])
    r_s, at_s = ux.worst_ratio(sg, s64, ux.prep_sigma_bound(s64))
    big, tiny = (z.cpu() > 20)[v], (s64 <= ux.SIGMA_MIN)[v]
    show(f'prep {name}', xs=r_xs, z=r_z, sigma=r_s, z_above_20=float(big.float().mean()), clamped=float(tiny.float().mean()))
    assert r_s <= 1, f'sigma: {r_s:.3g} x the bound at {at_s}'
    assert bool((sg.cpu()[~v] == 1).all()) and float(sg.min()) >= ux.SIGMA_MIN
    if name == 'large_z':
        assert bool(big.all()) and torch.equal(sg.cpu()[v], z.cpu()[v])           # softplus is the identity beyond 20
    if name == 'tiny_softplus':
        assert bool(tiny.all()) and bool((sg.cpu()[v] == ux.SIGMA_MIN).all())
    if name == 'straddle':
        assert 0.02 < float(big.float().mean()) < 0.9 and 0.02 < float(tiny.float().mean()) < 0.9


def test_symbol_backward_elementwise(lib):
    p = ux.sym_bwd_inputs()
    B, L = p['B'], p['L']
    g = torch.Generator().manual_seed(5)
    base_wr, base_br = ux.dyadic(g, (D,), 64, 16), ux.dyadic(g, (1,), 64, 16)
    out, dz, dwr, dbr = filled(B, L, D), filled(B, L), dev(base_wr).clone(), dev(base_br).clone()
    lib.dx_upsample_sym_bwd(*(P(dev(p[k])) for k in ('dxs_in', 'dsigma', 'xs', 'z', 'dur')), P(i32(p['lens'])),
                            *(P(dev(p[k])) for k in ('wd', 'bd', 'wr')), P(out), P(dz), P(dwr), P(dbr), B, L, D, S())
    torch.cuda.synchronize()
    v = ux.valid_mask(p['lens'], L)
    dz64, cmp = ux.sym_dz(p)
    assert int((~cmp).sum()) <= ux.MAX_EXCLUDED * int(v.sum())
    r_dz, at = ux.worst_ratio(dz, dz64, 8 * ux.U * dz64.abs(), cmp)
    assert r_dz <= 1, f'dz: {r_dz:.3g} x the bound at {at}, z = {float(p["z"][at]):.9g}'
    assert float(dz.cpu()[~v].abs().max()) == 0
    o64, w64, b64 = ux.sym_rest(p, dz)
    b_out, b_wr, b_br = ux.sym_bounds(p, dz)
    rows = B * L
    chain = 4 + -(-rows // (4 * ux.SYM_BWD_BLOCKS)) + 2 + ux.SYM_BWD_BLOCKS + 2     # the accumulated outputs' bounds include the base
    r_o, at_o = ux.worst_ratio(out, o64, b_out)
    r_w, at_w = ux.worst_ratio(dwr, base_wr.double() + w64, b_wr + chain * ux.U * base_wr.double().abs())
    r_b, _ = ux.worst_ratio(dbr, base_br.double() + b64, b_br + chain * ux.U * base_br.double().abs())
    show('symbol backward', dz=r_dz, dxs_out=r_o, dwr=r_w, dbr=r_b, excluded=int((~cmp).sum()))
    assert r_o <= 1, f'dxs_out: {r_o:.3g} x the bound at {at_o}'
    assert r_w <= 1 and r_b <= 1, f'dwr {r_w:.3g} (at {at_w}), dbr {r_b:.3g} x their summation bounds'
    assert torch.equal(out.cpu()[~v], p['dxs_in'][~v])


# ---- loss -----------------------------------------------------------------------------------------------------------------------------
def edge_name(c, b, t):
    names = []
    if t in (61, 62, 63, 64, 65, 66):
        names.append('the pooling window at t = 63/64 (block edge of the mel kernels)')
    if t in (253, 254, 255, 256, 257, 258):
        names.append('the pooling window at t = 255/256 (block edge of energy_diff)')
    if c['rows_exist'] is not None and abs(t - c['rows_exist'][b]) <= 2:
        names.append(f"the pooling window at rows_exist = {c['rows_exist'][b]}")
    if abs(t - c['lens'][b]) <= 2:
        names.append(f"the length edge {c['lens'][b]}")
    return ', '.join(names) or 'no edge'


def mel_grad(lib, c, ep, des, scale=1.0, scale_dev=None):
    B, M, T = c['B'], c['M'], c['T']
    dmel = filled(B, M, T)
    k = [ux.f32(c[n] * scale) for n in ('c_l1', 'c_l2', 'c_e')]
    head = (P(dev(c['mp'])), P(dev(c['mt'])), P(ep), P(des), P(i32(c['lens'])), *k, c['e_per_total'])
    if scale_dev is None:
        lib.dx_mel_grad(*head, P(dmel), B, M, T, S())
    else:
        lib.dx_mel_grad_dyn(*head, P(scale_dev), P(dmel), B, M, T, S())
    torch.cuda.synchronize()
    return dmel


@pytest.mark.parametrize('name', list(ux.LOSS_CASES))
def test_mel_and_energy_kernels_elementwise(lib, name):
    c = ux.loss_case(name)
    B, M, T = c['B'], c['M'], c['T']
    lens = i32(c['lens'])
    ep, et, l1, l2 = filled(B, T), filled(B, T), torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    lib.dx_mel_stats(P(dev(c['mp'])), P(dev(c['mt'])), P(ep), P(et), P(l1), P(l2), B, M, T, S())
    torch.cuda.synchronize()
    ref = ux.mel_stats_ref(c['mp'], c['mt'])
    bounds = ux.mel_stats_bounds(ref, M, T)
    r = {}
    for k, got in (('ep', ep), ('et', et), ('l1', l1), ('l2', l2)):
        r[k], at = ux.worst_ratio(got, ref[k], bounds[k])
        assert r[k] <= 1, f'{k}: {r[k]:.3g} x the bound at {at}' + (f' ({edge_name(c, *at)})' if len(at) == 2 else '')
    # energy_diff on the device's own energies; frames at and beyond rows_exist poisoned (they are the pooling's zero padding)
    ep_p, et_p = ep.clone(), et.clone()
    for b, n in enumerate(c['rows_exist'] or ()):
        ep_p[b, n:] = float('nan')
        et_p[b, n:] = float('nan')
    des, esum = filled(B, T), torch.zeros(1, device=DEV)
    lib.dx_energy_diff(P(ep_p), P(et_p), P(lens), P(des), P(esum), B, T, P(i32(c['rows_exist'])), S())
    torch.cuda.synchronize()
    des64, esum64, _ = ux.energy_ref(ep_p, et_p, c['lens'], c['rows_exist'])
    b_des, b_esum = ux.energy_bounds(ep_p, et_p, c['lens'], c['rows_exist'])
    r['des'], at = ux.worst_ratio(des, des64, b_des)
    assert r['des'] <= 1, f"des: {r['des']:.3g} x the bound at {at} ({edge_name(c, *at)})"
    r['esum'], _ = ux.worst_ratio(esum, esum64, b_esum)
    assert r['esum'] <= 1, f"esum: {r['esum']:.3g} x its chain bound"
    # mel_grad on the device's ep and des
    dmel = mel_grad(lib, c, ep, des)
    dmel64, b_dmel = ux.mel_grad_ref(c, ep, des)
    r['dmel'], at = ux.worst_ratio(dmel, dmel64, b_dmel)
    assert r['dmel'] <= 1, f"dmel: {r['dmel']:.3g} x the bound at {at} ({edge_name(c, at[0], at[2])})"
    for t in (t for t in (63, 64, 255, 256) if t < T):                      # the windows that cross a block edge, by name
        for what, rr in (('des', ux.worst_ratio(des[:, t], des64[:, t], b_des[:, t])[0]), ('dmel', ux.worst_ratio(dmel[:, :, t], dmel64[:, :, t], b_dmel[:, :, t])[0])):
            assert rr <= 1, f'{what}: {rr:.3g} x the bound in {edge_name(c, 0, t)}'
    show(f'loss {name}', **r)
    # the dynamic entry equals the static one given coefficient x scale, bit for bit
    for scale in (2.0 ** -3, 2.0 ** 15):
        s_dev = torch.full((1,), scale, dtype=torch.float32, device=DEV)
        assert torch.equal(mel_grad(lib, c, ep, des, 1.0, s_dev), mel_grad(lib, c, ep, des, scale)), f'dx_mel_grad_dyn, scale {scale}'


@pytest.mark.parametrize('ld', [1, 4])
@pytest.mark.parametrize('name', list(ux.PITCH_CASES))
def test_pitch_kernels_elementwise(lib, name, ld):
    """ld = 4: the (B, T, 4) rows the predictor's last convolution writes; channel 0 is read and written, the others must survive"""
    B, T, lens = ux.PITCH_CASES[name]
    for unvoiced in (False, True):
        c = ux.pitch_inputs(B, T, lens, all_unvoiced=unvoiced)
        L = i32(lens)
        pp = filled(B, T, ld)
        pp[:, :, 0] = dev(c['pp'])
        sums = torch.zeros(2, device=DEV)
        lib.dx_pitch_mse(P(pp), ld, P(dev(c['gt'])), P(L), P(sums), B, T, S())
        torch.cuda.synchronize()
        s64, n64, b = ux.pitch_ref(c)
        assert float(sums[1]) == n64
        r_s, _ = ux.worst_ratio(sums[:1], s64.reshape(1), b)
        assert r_s <= 1, f'pitch sum: {r_s:.3g} x its chain bound'

        def grad(scale, scale_dev=None):
            dpp = filled(B, T, ld)
            if scale_dev is None:
                lib.dx_pitch_grad(P(pp), ld, P(dev(c['gt'])), P(L), P(sums), scale, P(dpp), ld, B, T, S())
            else:
                lib.dx_pitch_grad_dyn(P(pp), ld, P(dev(c['gt'])), P(L), P(sums), scale, P(scale_dev), P(dpp), ld, B, T, S())
            torch.cuda.synchronize()
            return dpp
        dpp = grad(0.15)
        g64, bg = ux.pitch_grad_ref(c, float(sums[1]), 0.15)
        r_g, at = ux.worst_ratio(dpp[:, :, 0], g64, bg)
        assert r_g <= 1, f'pitch gradient: {r_g:.3g} x the bound at {at}'
        assert bool((dpp[:, :, 1:] == SENTINEL).all()) and bool((pp[:, :, 1:] == SENTINEL).all()), 'channels 1 to 3 did not survive'
        if unvoiced:
            assert float(sums.abs().max()) == 0 and float(dpp[:, :, 0].abs().max()) == 0
        else:
            show(f'pitch {name}, ld {ld}', sum=r_s, grad=r_g)
            for scale in (2.0 ** -3, 2.0 ** 15):
                s_dev = torch.full((1,), scale, dtype=torch.float32, device=DEV)
                assert torch.equal(grad(0.15, s_dev), grad(ux.f32(ux.f32(0.15) * scale))), f'dx_pitch_grad_dyn, scale {scale}'


def finalize(lib, f, off, gs_scale=1.0, scale_dev=None):
    B = f['B']
    t = {k: (None if k == off else dev(f[k])) for k in ('ce', 'pm', 'esum', 'psum')}
    dl = None if off == 'ce' else dev(f['dlogits'])
    d_spk = None if dl is None else filled(*dl.shape)
    d_pm = None if t['pm'] is None else filled(*t['pm'].shape)
    out = filled(8)
    args = (P(t['ce']), None, f['spk_w'], P(dl), P(d_spk), 0 if dl is None else dl.numel(), P(t['pm']), P(d_pm), 0 if d_pm is None else d_pm.numel(),
            f['pmw'], P(dev(f['l1sum'])), P(dev(f['l2sum'])), P(i32(f['lens'])), B, f['M'], f['msw'], P(t['esum']), f['ecw'], P(t['psum']), f['pcw'],
            P(out), P(out[7:]), ux.f32(f['grad_scale'] * gs_scale))
    if scale_dev is None:
        lib.dx_loss_finalize(*args, S())
    else:
        lib.dx_loss_finalize_dyn(*args, P(scale_dev), S())
    torch.cuda.synchronize()
    return {'terms': out[:7], 'total': out[7:], 'd_spk': d_spk, 'd_pm': d_pm}


@pytest.mark.parametrize('B', [3, 300])
@pytest.mark.parametrize('off', ux.FINALIZE_SWITCHES)
def test_loss_finalize_terms_total_and_null_switches(lib, B, off):
    f = ux.finalize_inputs(B, [1 + (5 * b) % 7 for b in range(B)])
    got, ref = finalize(lib, f, off), ux.finalize_ref(f, off)
    r = {}
    for k, (want, bound) in ref.items():
        r[k], at = ux.worst_ratio(got[k], want, bound)
        assert r[k] <= 1, f'{k}: {r[k]:.3g} x the bound at {at} with {off} NULL'
    show(f'finalize B={B}, {off} NULL', **r)
    idx = {'ce': (0, 1), 'pm': (2,), 'esum': (5,), 'psum': (6,)}.get(off, ())
    assert all(float(got['terms'][i]) == 0 for i in idx)
    if off is None:
        for scale in (2.0 ** -3, 2.0 ** 15):
            s_dev = torch.full((1,), scale, dtype=torch.float32, device=DEV)
            a, b = finalize(lib, f, off, 1.0, s_dev), finalize(lib, f, off, scale)
            assert all(torch.equal(a[k], b[k]) for k in a), f'dx_loss_finalize_dyn, scale {scale}'
            assert torch.equal(a['terms'], got['terms']) and torch.equal(a['total'], got['total'])      # the terms carry no scale


@pytest.mark.parametrize('B', [5, 257])
def test_cross_entropy_elementwise(lib, B):
    logits, target = ux.cross_entropy_inputs(B)
    loss, dl = filled(1), filled(B, 3)
    lib.dx_cross_entropy(P(dev(logits)), P(dev(target)), P(loss), P(dl), B, 3, S())
    torch.cuda.synchronize()
    loss64, dl64, b_loss, b_dl = ux.cross_entropy_ref(logits, target)
    r_l, _ = ux.worst_ratio(loss, loss64, b_loss)
    r_d, at = ux.worst_ratio(dl, dl64, b_dl)
    show(f'cross entropy B={B}', loss=r_l, dlogits=r_d)
    assert r_l <= 1 and r_d <= 1, f'loss {r_l:.3g}, dlogits {r_d:.3g} x the bound (at {at})'
