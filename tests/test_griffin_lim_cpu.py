"""Griffin-Lim without a GPU: the library's new entry points and their argument checks, the float64 restatement against the reference
signals of tests/golden/griffin_lim.npz, the packing of the filter bank, and the float32 FISTA against the reference's NNLS residual."""
import ctypes

import numpy as np
import pytest

from tests import griffin_lim_helpers as gh
from ubisoft_laforge_daft_exprt_amd import griffin_lim as gl
from ubisoft_laforge_daft_exprt_amd.mel import mel_filter_bank

FMAX = (8000.0, None)


@pytest.fixture(scope='module')
def g():
    return gh.golden()


def test_library_and_package_export_the_new_symbols():
    import ubisoft_laforge_daft_exprt_amd as dx
    from ubisoft_laforge_daft_exprt_amd import _lib
    protos = _lib.parse_header()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('dx_gl_iter', 'dx_gl_layout', 'dx_gl_peak_normalize', 'dx_nnls_mel'):
        assert name in protos and hasattr(dll, name), name
    assert _lib.lib().dx_version() == 1
    tile, words = gl.layout()
    assert words == gl.PACK_WORDS and tile >= 4
    for name in ('GriffinLim', 'GriffinLimVocoder', 'griffin_lim_reconstruction_from_mel_spec'):
        assert hasattr(dx, name), name


def test_argument_validation_without_gpu():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    with pytest.raises(DxError, match='null'):
        L.dx_gl_iter(None, None, 2048, None, 513, None, None, 1, 1, 1024, 256, None)
    with pytest.raises(DxError, match='1024'):
        L.dx_gl_iter(16, 32, 2048, 16, 513 * 4, 16, 16, 1, 4, 2048, 256, None)
    with pytest.raises(DxError, match='1024'):
        L.dx_gl_iter(16, 32, 2048, 16, 513 * 4, 16, 16, 1, 4, 1024, 128, None)
    with pytest.raises(DxError, match='alias'):
        L.dx_gl_iter(16, 16, 2048, 16, 513 * 4, 16, 16, 1, 4, 1024, 256, None)
    with pytest.raises(DxError, match='shape'):
        L.dx_gl_iter(16, 32, 2048, 16, 513 * 4, 16, 16, 65536, 4, 1024, 256, None)
    with pytest.raises(DxError, match='strides'):
        L.dx_gl_iter(16, 32, 2047, 16, 513 * 4, 16, 16, 1, 4, 1024, 256, None)     # 256 * 4 + 1024 = 2048 samples are needed
    with pytest.raises(DxError, match='aligned'):
        L.dx_gl_iter(16, 36, 2048, 16, 513 * 4, 16, 16, 1, 4, 1024, 256, None)
    with pytest.raises(DxError, match='null'):
        L.dx_gl_peak_normalize(None, None, 8, 1, 8, None)
    with pytest.raises(DxError, match='shape'):
        L.dx_gl_peak_normalize(16, 16, 4, 1, 8, None)
    with pytest.raises(DxError, match='null'):
        L.dx_nnls_mel(None, 80, None, None, None, 1.0, 200, None, 513, 1, 1, 80, 513, None)
    with pytest.raises(DxError, match='513'):
        L.dx_nnls_mel(16, 80, 16, 16, 16, 1.0, 200, 16, 513, 1, 1, 80, 512, None)
    with pytest.raises(DxError, match='strides'):
        L.dx_nnls_mel(16, 79, 16, 16, 16, 1.0, 200, 16, 513, 1, 1, 80, 513, None)
    # the host side: geometry and device are checked before anything is launched
    hp = lambda **kw: type('HP', (), kw)()
    with pytest.raises(NotImplementedError):
        gl.GriffinLim(hp(filter_length=2048))
    with pytest.raises(NotImplementedError):
        gl.GriffinLim(hp(hop_length=128))
    import torch
    cpu = gl.GriffinLim(device='cpu')
    with pytest.raises(RuntimeError, match='GPU'):
        cpu.reconstruct(torch.zeros(1, 513, 4), [4])
    with pytest.raises(RuntimeError, match='GPU'):
        cpu.from_mel(torch.zeros(1, 80, 4), [4])
    with pytest.raises(ValueError):
        cpu.mel_to_linear(torch.zeros(1, 79, 4), [4])


def test_tables_are_double_rounded_once():
    tab = gl.gl_tables()
    assert tab.dtype == np.float32 and tab.shape == (3072,)
    assert np.array_equal(tab[:1024], np.hanning(1024).astype(np.float32))          # symmetric: zero at both ends
    assert tab[0] == 0 and tab[1023] == 0
    for ns in (4, 16, 64, 256):
        for r in (1, 2, 3):
            o = ns - 4 + (r - 1) * ns
            ang = 2 * np.pi * np.arange(ns) * r / (4 * ns)
            assert np.array_equal(tab[1024 + o:1024 + o + ns], np.cos(ang).astype(np.float32))
            assert np.array_equal(tab[2048 + o:2048 + o + ns], (-np.sin(ang)).astype(np.float32))


def test_float64_restatement_equals_every_reference_signal(g):
    M = g['speech/nnls'][:, :-2].astype(np.float64)
    S = 256 * M.shape[1] + 1024
    for start_name in gh.STARTS:
        start = g['noise'] if start_name == 'noise' else np.zeros(S, dtype=np.float32)
        _, kept = gh.gl_iterate(M, start, max(gh.ITERS), np.float64, keep=gh.ITERS)
        for k in gh.ITERS:
            ref = g[f'gl/{start_name}/{k}']
            assert ref.shape == (S,) and ref.dtype == np.float64
            d = np.abs(kept[k] - ref).max()
            print(f'{start_name} {k}: |restatement - reference| max {d:.1e}')
            assert d <= 1e-12, (start_name, k, d)
            assert not ref[-256:].any()                                             # the last hop is touched by no frame
    assert abs(gh.spectral_convergence(gh.gl_iterate(M, g['noise'], 128), M) - float(g['gl/convergence'])) <= 1e-9


@pytest.mark.parametrize('fmax', FMAX)
def test_bank_packing_round_trips(fmax):
    A = mel_filter_bank(22050, 1024, 80, 0.0, fmax)
    bank = gl.pack_filter_bank(A)
    assert bank['pack'].dtype == np.int32 and bank['pack'].shape == (gl.PACK_WORDS,)
    assert np.array_equal(gh.unpack_bins(bank['pack'], 80), A)
    assert np.array_equal(gh.unpack_channels(bank['pack'], 80), A)
    # pinv and the step come from double: equal to the double results rounded once, and better than their float32 computations
    A64 = A.astype(np.float64)
    assert bank['pinv_t'].shape == (80, gl.KP) and not bank['pinv_t'][:, 513:].any()
    assert np.array_equal(bank['pinv_t'][:, :513], np.linalg.pinv(A64).T.astype(np.float32))
    assert bank['step'] == 1.0 / np.linalg.norm(A64, 2) ** 2
    assert np.abs(A64 @ bank['pinv_t'][:, :513].T.astype(np.float64) - np.eye(80)).max() < 1e-5


def test_bank_packing_rejects_other_structures():
    A = mel_filter_bank(22050, 1024, 80, 0.0, 8000.0)
    three = A.copy()
    k = int(np.argmax((A != 0).sum(axis=0) == 2))
    free = [n for n in range(80) if three[n, k] == 0][:1]
    three[free[0], k] = 0.5
    with pytest.raises(ValueError, match='at most two'):
        gl.pack_filter_bank(three)
    gap = A.copy()
    ks = np.flatnonzero(gap[40])
    assert ks.size >= 3
    gap[40, ks[1]] = 0.0
    with pytest.raises(ValueError, match='consecutive'):
        gl.pack_filter_bank(gap)
    with pytest.raises(ValueError):
        gl.pack_filter_bank(A[:, :512])


def test_float32_fista_reaches_the_reference_residual(g):
    A = mel_filter_bank(22050, 1024, 80, 0.0, 8000.0)
    for name in ('speech', 'chirp'):
        m = np.exp(g[f'{name}/mel'])
        X = gh.fista32(A, m, 200)
        res, ref = gh.relative_residual(A, X, m), float(g[f'{name}/residual'])
        print(f'{name}: float32 FISTA residual {res:.2e}, reference {ref:.2e}')
        assert (X >= 0).all() and res <= ref, (name, res, ref)
        assert abs(gh.relative_residual(A, g[f'{name}/nnls'], m) - ref) <= 1e-3 * ref    # the stored solution is the one the residual is of
