"""Host side of the dynamic fp16 loss scaler: hparams validation, the checkpoint entry, the C ABI's argument checks and exports.
No GPU work: every call here must fail (or succeed) before any launch."""
import ctypes

import pytest
import torch

NEW_ENTRY_POINTS = ('dx_scaler_update', 'dx_adam_step_dyn', 'dx_mel_grad_dyn', 'dx_pitch_grad_dyn', 'dx_loss_finalize_dyn')


def test_hparams_defaults_are_gradscalers_and_static_by_default():
    from ubisoft_laforge_daft_exprt_amd.hparams import HyperParams, loss_scale_config
    cfg = loss_scale_config(HyperParams())
    assert cfg == {'dynamic': False, 'loss_scale': 4096.0, 'growth_interval': 2000, 'growth': 2.0, 'backoff': 0.5, 'min': 1.0, 'max': 2.0 ** 24}
    # any attribute bag serves (the reference's own HyperParams, an argparse.Namespace): missing keys take the defaults
    import argparse
    assert loss_scale_config(argparse.Namespace(loss_scale=512)) == {**cfg, 'loss_scale': 512.0}
    # the static scale may be any positive number, as before
    assert loss_scale_config(HyperParams(loss_scale=3000.0))['loss_scale'] == 3000.0


@pytest.mark.parametrize('bad', [dict(dynamic_loss_scale=True, loss_scale=3000.0), dict(dynamic_loss_scale=True, loss_scale=0.0),
                                 dict(loss_scale_growth=3.0), dict(loss_scale_growth=0.5), dict(loss_scale_backoff=0.3),
                                 dict(loss_scale_backoff=2.0), dict(loss_scale_growth_interval=0), dict(loss_scale_growth_interval=2.5),
                                 dict(loss_scale_min=0.0), dict(loss_scale_min=8.0, loss_scale_max=4.0),
                                 dict(dynamic_loss_scale=True, loss_scale=2.0 ** 30),                      # beyond loss_scale_max
                                 dict(dynamic_loss_scale=True, loss_scale=0.5)])                           # below loss_scale_min
def test_hparams_validation_rejects_what_is_no_power_of_two_or_out_of_range(bad):
    from ubisoft_laforge_daft_exprt_amd.hparams import HyperParams
    with pytest.raises(ValueError, match='loss_scale'):
        HyperParams(**bad)
    with pytest.raises(ValueError, match='loss_scale'):
        HyperParams().clone(**bad)


def test_hparams_accepts_every_power_of_two():
    from ubisoft_laforge_daft_exprt_amd.hparams import HyperParams
    hp = HyperParams(dynamic_loss_scale=True, loss_scale=2.0 ** 40, loss_scale_max=2.0 ** 40, loss_scale_min=2.0 ** -10, loss_scale_growth=4.0,
                     loss_scale_backoff=0.25, loss_scale_growth_interval=3)
    from ubisoft_laforge_daft_exprt_amd.hparams import loss_scale_config
    assert loss_scale_config(hp) == {'dynamic': True, 'loss_scale': 2.0 ** 40, 'growth_interval': 3, 'growth': 4.0, 'backoff': 0.25,
                                     'min': 2.0 ** -10, 'max': 2.0 ** 40}
    assert loss_scale_config(hp.clone(loss_scale=2.0 ** -3))['loss_scale'] == 0.125
    # the keys are attributes only when given: a checkpoint's ``config_params`` stay what they were for a run that sets none
    assert not any(k.startswith('loss_scale') or k == 'dynamic_loss_scale' for k in vars(HyperParams()))


def test_header_declares_and_library_exports_the_new_entry_points():
    from ubisoft_laforge_daft_exprt_amd import _lib
    protos = _lib.parse_header(with_names=True)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert name in protos, name
        assert hasattr(dll, name), name
        assert protos[name][2][-1] == 'stream'                   # launches on the caller's stream
    assert 'scale_dev' in protos['dx_mel_grad_dyn'][2] and 'scale_dev' in protos['dx_pitch_grad_dyn'][2] and 'scale_dev' in protos['dx_loss_finalize_dyn'][2]
    # the static entry points keep their signatures
    assert 'scale_dev' not in protos['dx_mel_grad'][2] and len(protos['dx_adam_step'][2]) == 18


def test_new_entry_points_are_priced():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[5, 9, 12]])
    assert profiling.price('dx_adam_step_dyn', {'n': 1000}, geom) == ('adam_dyn_kernel', 'hbm', None, 28000)
    assert profiling.price('dx_scaler_update', {}, geom)[3] == 68
    assert profiling.price('dx_mel_grad_dyn', {'B': 3, 'M': 80, 'T': 12}, geom) == profiling.price('dx_mel_grad', {'B': 3, 'M': 80, 'T': 12}, geom)


def test_null_pointers_and_bad_sizes_raise_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    P = 4096                                                     # a non-null, aligned address that is never dereferenced: the checks come first
    ok_scaler = (0.9, 0.98, 2.0, 0.5, 3, 1.0, 2.0 ** 24, None)
    for state, normsq in ((None, P), (P, None)):
        with pytest.raises(DxError, match='null'):
            L.dx_scaler_update(state, normsq, *ok_scaler)
    for bad in ((0.9, 0.98, 3.0, 0.5, 3, 1.0, 16.0, None), (0.9, 0.98, 2.0, 0.3, 3, 1.0, 16.0, None), (0.9, 0.98, 2.0, 0.5, 0, 1.0, 16.0, None),
                (0.9, 0.98, 2.0, 0.5, 3, 32.0, 16.0, None), (1.0, 0.98, 2.0, 0.5, 3, 1.0, 16.0, None)):
        with pytest.raises(DxError):
            L.dx_scaler_update(P, 2 * P, *bad)
    with pytest.raises(DxError, match='distinct'):
        L.dx_scaler_update(P, P, *ok_scaler)
    adam = lambda p=P, g=P, m=P, v=P, n=8, normsq=P, scaler=P, zero_after=None: L.dx_adam_step_dyn(
        p, g, m, v, n, 1e-3, 0.9, 0.98, 1e-9, 1e-6, normsq, float('inf'), scaler, None, zero_after, None)
    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(normsq=None), dict(scaler=None), dict(n=0), dict(n=-4)):
        with pytest.raises(DxError, match='null'):
            adam(**kw)
    with pytest.raises(DxError, match='alias'):
        adam(zero_after=P)
    with pytest.raises(DxError, match='aligned'):
        adam(p=P + 4)
    mel = lambda mp=P, mt=P, lens=P, scale=P, dmel=P, B=1, T=4: L.dx_mel_grad_dyn(mp, mt, None, None, lens, 1.0, 1.0, 0.0, 0, scale, dmel, B, 80, T, None)
    for kw in (dict(mp=None), dict(mt=None), dict(lens=None), dict(scale=None), dict(dmel=None), dict(B=0), dict(T=-1)):
        with pytest.raises(DxError, match='null'):
            mel(**kw)
    with pytest.raises(DxError, match='energy'):
        L.dx_mel_grad_dyn(P, P, None, None, P, 1.0, 1.0, 0.5, 0, P, P, 1, 80, 4, None)
    pitch = lambda pp=P, gt=P, lens=P, sums=P, scale=P, dpp=P, B=1, T=4: L.dx_pitch_grad_dyn(pp, 1, gt, lens, sums, 1.0, scale, dpp, 1, B, T, None)
    for kw in (dict(pp=None), dict(gt=None), dict(lens=None), dict(sums=None), dict(scale=None), dict(dpp=None), dict(B=0), dict(T=0)):
        with pytest.raises(DxError, match='null'):
            pitch(**kw)
    fin = lambda l1=P, l2=P, lens=P, terms=P, total=P, scale=P, B=1: L.dx_loss_finalize_dyn(
        None, None, 0.0, None, None, 0, None, None, 0, 0.0, l1, l2, lens, B, 80, 1.0, None, 0.0, None, 0.0, terms, total, 1.0, scale, None)
    for kw in (dict(l1=None), dict(l2=None), dict(lens=None), dict(terms=None), dict(total=None), dict(scale=None), dict(B=0)):
        with pytest.raises(DxError, match='null'):
            fin(**kw)
    with pytest.raises(DxError, match='speaker'):
        L.dx_loss_finalize_dyn(None, None, 0.0, None, None, 3, None, None, 0, 0.0, P, P, P, 1, 80, 1.0, None, 0.0, None, 0.0, P, P, 1.0, P, None)


def test_checkpoint_entry_round_trips_and_old_checkpoints_load():
    """The ``loss_scaler`` entry is four plain numbers: it survives ``torch.save`` / ``torch.load(weights_only=True)`` (how
    Trainer.load_checkpoint reads a file) and LossScaler.load writes exactly those words; without the entry the scale starts from
    ``hparams.loss_scale`` and the bias-correction step from the optimiser state."""
    import io
    from ubisoft_laforge_daft_exprt_amd.hparams import HyperParams, loss_scale_config
    from ubisoft_laforge_daft_exprt_amd.optim import LossScaler, ScalerState
    cfg = loss_scale_config(HyperParams(dynamic_loss_scale=True, loss_scale=1024.0))
    sc = LossScaler(cfg, 'cpu')                                   # the host logic needs no GPU: the state words are a plain tensor
    assert dict(ScalerState(sc.words.clone()).items()) == {'scale': 1024.0, 'applied': 0, 'good_steps': 0, 'skipped': 0}
    entry = {'scale': 256.0, 'applied': 17, 'good_steps': 2, 'skipped': 3}
    buf = io.BytesIO()
    torch.save({'iteration': 20, 'loss_scaler': entry}, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)
    assert back['loss_scaler'] == entry and all(type(v) in (int, float) for v in back['loss_scaler'].values())
    ptr = sc.words.data_ptr()
    sc.load(back['loss_scaler'])
    assert sc.words.data_ptr() == ptr                             # in place: captured graphs hold the pointer
    state = ScalerState(sc.words.clone())
    assert len(state) == 4 and 'scale' in state and dict(state.items()) == entry
    assert float(sc.scale) == 256.0
    assert sc.words[[1, 2, 6, 7]].tolist() == [0, 0, 0, 0]        # the words the decision launch writes before anything reads them
    # a checkpoint without the entry (Trainer.load_checkpoint passes the optimiser's step on)
    sc.load({'applied': 17})
    assert dict(ScalerState(sc.words.clone()).items()) == {'scale': 1024.0, 'applied': 17, 'good_steps': 0, 'skipped': 0}
    for bad in (300.0, 2.0 ** 30, 0.25):
        with pytest.raises(ValueError, match='power of two'):
            sc.load({'scale': bad})


def test_loss_accepts_a_host_factor_and_device_scalar_pair_only_on_the_gpu():
    from ubisoft_laforge_daft_exprt_amd import ops
    with pytest.raises(TypeError, match='float32'):
        ops._scale_dev(torch.ones(1))                             # a CPU tensor is no device scalar
    with pytest.raises(TypeError, match='float32'):
        ops._scale_dev(4096.0)
