"""CPU checks of the mel backward's fixture and C ABI: the fp64 restatement reproduces the stored gradients, the reference's fp32
gradients lie within their stored spread, few cells are taken out near the clamp, the library exports dx_mel_bwd as the header
declares it, and the profiler prices it."""
import os
import re

import numpy as np
import pytest

from tests import mel_grad_helpers as gh
from tests import mel_helpers as mh
from ubisoft_laforge_daft_exprt_amd import _lib, mel, profiling


@pytest.fixture(scope='module')
def golden():
    return gh.golden()


def test_fixture_covers_every_signal_of_the_forward_fixture(golden):
    assert list(golden) == list(mh.golden())
    for name, d in golden.items():
        n = len(d['wav'])
        for v in mh.FMAX:
            e = d[v]
            assert e['g'].shape == e['target'].shape == (80, n // 256) and e['g'].dtype == np.float32
            assert e['d64'].shape == e['dloss64'].shape == (n,) and e['d64'].dtype == e['dloss64'].dtype == np.float64
            assert e['d32_ref'].shape == e['dloss32_ref'].shape == (n,) and e['d32_ref'].dtype == e['dloss32_ref'].dtype == np.float32


@pytest.mark.parametrize('v', list(mh.FMAX))
def test_fp64_restatement_reproduces_the_stored_gradients(golden, v):
    for name, d in golden.items():
        e = d[v]
        fb = mel.mel_filter_bank(22050, 1024, 80, 0.0, mh.FMAX[v])
        d64 = gh.grad_fp64(d['wav'], fb, e['g'])
        assert np.abs(d64 - e['d64']).max() <= 1e-10 * np.abs(e['d64']).max(), (name, v)
        loss64, dl64 = gh.loss_fp64(d['wav'], fb, e['target'])
        assert abs(loss64 - float(e['loss64'])) <= 1e-10 * abs(float(e['loss64'])), (name, v)
        assert np.abs(dl64 - e['dloss64']).max() <= 1e-10 * np.abs(e['dloss64']).max(), (name, v)
        # the log-mel of the forward fixture is the same function
        assert np.allclose(gh.mel_fp64(d['wav'], fb), mh.golden()[name][v]['f64'], rtol=0, atol=1e-9)


def test_reference_fp32_gradients_lie_within_their_stored_spread(golden):
    for name, d in golden.items():
        for v in mh.FMAX:
            e = d[v]
            for ref, f64, spread in ((e['d32_ref'], e['d64'], e['spread']), (e['dloss32_ref'], e['dloss64'], e['loss_spread'])):
                dd = np.abs(ref - f64)
                assert dd.max() <= spread[0] * (1 + 1e-12) and dd.mean() <= spread[1] * (1 + 1e-12), (name, v)
                assert spread[0] > 0 and spread[0] < 5e-2 * np.abs(f64).max(), (name, v)
            assert abs(float(e['loss_ref']) - float(e['loss64'])) < 1e-5 * float(e['loss64']), (name, v)


def test_cells_zeroed_near_the_clamp_are_few_and_exactly_those(golden):
    for name, d in golden.items():
        for v, fmax in mh.FMAX.items():
            e = d[v]
            near = gh.near_clip(gh.lin_fp64(d['wav'], mel.mel_filter_bank(22050, 1024, 80, 0.0, fmax)))
            assert float(e['share']) == near.mean() <= 0.01, (name, v, float(e['share']))
            assert not e['g'][near].any() and (e['g'][~near] != 0).all(), (name, v)


def test_library_exports_the_backward_as_the_header_declares_it():
    protos = _lib.parse_header(with_names=True)
    assert 'dx_mel_bwd' in protos and 'dx_mel_bwd_pack' in protos
    names = protos['dx_mel_bwd'][2]
    assert names[:4] == ['wav', 'sxb', 'S', 'lengths'] and {'gmel', 'dwav', 'clip', 'stream'} <= set(names)
    assert os.path.exists(_lib.LIB_PATH), 'build the library first'
    import ctypes
    dll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, 'dx_mel_bwd') and hasattr(dll, 'dx_mel_bwd_pack')
    src = open(os.path.join(_lib.PKG, 'csrc', 'dx_mel.hip')).read()
    body = src[src.index('int dx_mel_bwd('):]
    assert re.search(r'DX_REQUIRE', body[:body.index('hipStream_t')]), 'host checks run before the launch'
    assert 'atomicAdd' not in src and 'atomic_' not in src


def test_backward_launch_is_priced_as_mfma_on_valid_frames_only():
    frames = [129, 40, 3]
    geom = profiling.Geometry([frames])
    a = dict(B=3, T_max=129, n_mels=80, kmax=372, S=33054, sxb=33054, sgb=80 * 129)
    label, bound, flops, byt = profiling.price('dx_mel_bwd', a, geom)
    assert label == 'mel_bwd<f32>' and bound == 'mfma' and byt > 0
    assert flops == 2 * profiling.price('dx_mel', a, geom)[2]      # the forward's two GEMMs recomputed + their two transposes
    assert profiling.price('dx_mel_bwd_pack', dict(n_mels=80, n_freq=513, kmax=372), geom)[1] == 'hbm'
