"""Hyper-parameters that shape the acoustic-model hot path.

Only the keys the model / loss / duration math read are kept (reference:
src/daft_exprt/hparams.py:36-127 for the defaults, model.py:838-856 and
loss.py:22-50 for the keys that are actually consumed).  File-system, MFA,
feature-extraction and trainer keys of the reference's ``HyperParams`` are out
of scope and deliberately absent.

Any object exposing the same attribute names (for instance the reference's
own ``HyperParams`` instance, or an ``argparse.Namespace`` built from a
``config.json``) can be handed to ``DaftExprt`` / ``DaftExprtLoss`` instead.
"""
from __future__ import annotations

import copy
import math

N_SYMBOLS_ENGLISH = 76  # len(symbols_english), reference symbols.py:16-36 (pad '_' at index 0)


def _fft_stack(nb_blocks=4, hidden=128, heads=2, conv_channels=1024, kernel=3, attn_dropout=0.1, conv_dropout=0.1):
    return {
        'nb_blocks': nb_blocks,
        'hidden_embed_dim': hidden,
        'attn_nb_heads': heads,
        'attn_dropout': attn_dropout,
        'conv_kernel': kernel,
        'conv_channels': conv_channels,
        'conv_dropout': conv_dropout,
    }


def _power_of_two(x) -> bool:
    x = float(x)
    return x > 0.0 and math.isfinite(x) and math.frexp(x)[0] == 0.5


def loss_scale_config(hparams) -> dict:
    """The fp16 loss-scaling keys of any hparams object, with the defaults for those it lacks, checked (ValueError):
    ``dynamic_loss_scale`` (False: the static scale ``loss_scale``), ``loss_scale`` (4096; the initial value in dynamic mode, where it
    must be a power of two), ``loss_scale_growth_interval`` (2000), ``loss_scale_growth`` (2.0) and ``loss_scale_backoff`` (0.5) -- the
    defaults of torch.amp.GradScaler, both powers of two -- and the bounds ``loss_scale_min`` (1.0) <= scale <= ``loss_scale_max``
    (2**24).  Every scale the dynamic scaler can reach is then a power of two: multiplying by it is exact."""
    g = lambda k, d: getattr(hparams, k, d)
    cfg = {'dynamic': bool(g('dynamic_loss_scale', False)), 'loss_scale': float(g('loss_scale', 4096.0)),
           'growth_interval': int(g('loss_scale_growth_interval', 2000)), 'growth': float(g('loss_scale_growth', 2.0)),
           'backoff': float(g('loss_scale_backoff', 0.5)), 'min': float(g('loss_scale_min', 1.0)), 'max': float(g('loss_scale_max', 2.0 ** 24))}
    if not (_power_of_two(cfg['growth']) and cfg['growth'] >= 1.0):
        raise ValueError(f"loss_scale_growth must be a power of two >= 1, got {cfg['growth']!r}")
    if not (_power_of_two(cfg['backoff']) and cfg['backoff'] <= 1.0):
        raise ValueError(f"loss_scale_backoff must be a power of two <= 1, got {cfg['backoff']!r}")
    if cfg['growth_interval'] < 1 or cfg['growth_interval'] != g('loss_scale_growth_interval', 2000):
        raise ValueError(f"loss_scale_growth_interval must be a positive integer, got {g('loss_scale_growth_interval', 2000)!r}")
    if not (0.0 < cfg['min'] <= cfg['max'] < math.inf):
        raise ValueError(f"need 0 < loss_scale_min <= loss_scale_max < inf, got {cfg['min']!r}, {cfg['max']!r}")
    if cfg['dynamic']:
        if not _power_of_two(cfg['loss_scale']):
            raise ValueError(f"dynamic_loss_scale: loss_scale must be a power of two, got {cfg['loss_scale']!r}")
        if not cfg['min'] <= cfg['loss_scale'] <= cfg['max']:
            raise ValueError(f"dynamic_loss_scale: loss_scale {cfg['loss_scale']!r} lies outside [loss_scale_min, loss_scale_max] = [{cfg['min']!r}, {cfg['max']!r}]")
    return cfg


class HyperParams:
    """Attribute bag with the reference's default values for the hot path."""

    def __init__(self, **kwargs):
        # mel / duration arithmetic (hparams.py:39-46)
        self.centered = False
        self.sampling_rate = 22050
        self.n_mel_channels = 80
        self.filter_length = 1024
        self.hop_length = 256
        # vocabulary / speakers (hparams.py:186-200)
        self.n_symbols = N_SYMBOLS_ENGLISH
        self.n_speakers = 2
        self.external_emb_dim = 192  # model.py:855
        # loss weights (hparams.py:71-88, loss.py:24-40)
        self.post_mult_weight = 1e-3
        self.mel_spec_weight = 1.0
        self.adv_max_weight = 1e-2
        self.warmup_steps = 10000
        self.energy_consistency_weight = 0.05
        self.pitch_consistency_weight = 0.15
        self.pitch_predictor_path = ''
        # optimiser / schedule (hparams.py:92-100; read by optim.FusedAdam, optim.update_learning_rate and train_steps.Trainer)
        self.accumulation_steps = 1
        self.betas = [0.9, 0.98]
        self.epsilon = 1e-9
        self.weight_decay = 1e-6
        self.grad_clip_thresh = float('inf')
        self.initial_learning_rate = 1e-4
        self.max_learning_rate = 1e-3
        # fp16 loss scaling (no reference counterpart) is read through loss_scale_config(), which holds the defaults: ``loss_scale``,
        # ``dynamic_loss_scale``, ``loss_scale_growth_interval`` / ``_growth`` / ``_backoff`` / ``_min`` / ``_max``.  They are attributes only
        # when given, so the ``config_params`` of a checkpoint are what they were unless a run sets one.
        # gradient reversal strength (model.py:51; not defined by the reference defaults)
        self.lambda_reversal = 1.0
        # module shapes (hparams.py:106-127)
        self.phoneme_encoder = _fft_stack()
        self.gaussian_upsampling_module = {'conv_kernel': 3}
        fd = _fft_stack()
        del fd['hidden_embed_dim']  # inserted by the decoder itself, model.py:534
        self.frame_decoder = fd
        # per-speaker statistics used by pitch_shift (model.py:984-985)
        self.stats = {}
        for key, value in kwargs.items():
            setattr(self, key, value)
        loss_scale_config(self)

    def clone(self, **overrides):
        new = copy.deepcopy(self)
        for key, value in overrides.items():
            setattr(new, key, value)
        loss_scale_config(new)
        return new

    def without_dropout(self):
        new = copy.deepcopy(self)
        for name in ('phoneme_encoder', 'frame_decoder', 'accent_encoder'):
            cfg = getattr(new, name, None)
            if cfg is not None:
                cfg['attn_dropout'] = 0.0
                cfg['conv_dropout'] = 0.0
        return new
