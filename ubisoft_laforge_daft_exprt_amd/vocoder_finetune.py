"""The HiFi-GAN fine-tuning loop on gfx950 (reference vocoder/finetune_hifigan.py:119-319 without TensorBoard): one call per step,
``fit`` for the loop around it on the device-resident data of vocoder_data.py, checkpoints in the reference's layout.

``train_step`` runs the reference's order (lines 203-245): the generator forward once and the mel of ``y_g_hat``; the discriminator
step on ``y_g_hat.detach()``; the generator step against the stepped discriminators.  Every gradient is this package's HIP; weight
norm (backward and fold) and both AdamW steps are one ``dx_wn_adamw`` launch per optimiser (vocoder_optim.NormedAdamW): the generator
runs from folded leaves the optimiser owns, the discriminators' packs are rebuilt from the optimiser's ``W``.  Only the eight
spectral-normed layers keep torch's ``W / sigma`` backward and fold (sigma's gradient is a reduction over the whole tensor).

Stated deviations from the reference: an optimiser state that does not fit raises ``ValueError`` (the reference starts fresh silently);
``disc_checkpoint=None`` raises (this package has no initialiser for the discriminators); ``step`` continues from the checkpoint's
``steps`` (the reference restarts its count at 0); ``epoch`` counts the ``end_epoch()`` calls, which is what the reference has written
into its final checkpoint, and a restored tuner's learning rates are ``initial_lr * lr_decay ** epoch``; a checkpoint ``fit`` writes
mid-pass therefore holds the completed passes, where the reference writes the 1-based pass in progress.

Not built (DESIGN.md sections 19 and 20): graph capture of the step, bf16 operands, more than one GPU, writing the operand packs from
the optimiser kernel, TensorBoard.
"""
from __future__ import annotations

import os
from typing import Dict, NamedTuple, Optional

import torch

from .discriminators import HiFiGanDiscriminators, _checkpoint
from .lazy import DeviceDict
from .mel import MelL1Loss
from .vocoder import HOP, HiFiGANGenerator, _checkpoint_state, config_from_state
from .vocoder_optim import NormedAdamW
from .vocoder_train import generator_forward_folded

LOSS_NAMES = ('loss_disc_f', 'loss_disc_s', 'loss_gen_f', 'loss_gen_s', 'loss_fm_f', 'loss_fm_s', 'loss_mel')


class StepLosses(DeviceDict):
    """The seven losses of one step, one fp32 device vector until somebody looks (then ONE host transfer)."""
    KEYS = LOSS_NAMES


class FitResult(NamedTuple):
    """What ``HiFiGanFineTuner.fit`` did: the steps it ran, the last step's losses (None if it ran none; still on the device) and the
    validation mel errors by step count."""
    steps: int
    losses: Optional[StepLosses]
    validation: Dict[int, float]


def _layers(prefix, module):
    """(name, layer) for every layer of ``module`` in the order of ``module.parameters()``: the modules that own a bias."""
    return [(prefix + name, m) for name, m in module.named_modules() if 'bias' in dict(m.named_parameters(recurse=False))]


def _decayed(lr, gamma, epochs):
    for _ in range(int(epochs)):                     # as torch's ExponentialLR steps it: one multiplication per epoch
        lr = lr * gamma
    return lr


class HiFiGanFineTuner:
    """``gen_checkpoint``: a generator checkpoint (path or dict, V1 / V2 / V3 as ``HiFiGanVocoder.from_checkpoint`` reads them, weight
    norm intact); ``disc_checkpoint``: a reference ``do_*`` file or dict.  With ``reset_optimizers=False`` a ``disc_checkpoint`` that
    carries ``optim_g`` / ``optim_d`` restores both optimisers, ``steps`` and ``epoch`` (lines 139-152).

    Public: ``generator``, ``discriminators`` (HiFiGanDiscriminators), ``optim_g``, ``optim_d``, ``step``, ``epoch``."""

    def __init__(self, gen_checkpoint, disc_checkpoint, device='cuda', config=None, learning_rate=2e-4, adam_b1=0.8, adam_b2=0.99,
                 lr_decay=0.999, reset_optimizers=False, power_iterations=1, precision='f32'):
        if precision != 'f32':
            raise ValueError(f"HiFiGanFineTuner: gradients exist for precision 'f32' only, got {precision!r}")
        if gen_checkpoint is None:
            raise ValueError('HiFiGanFineTuner: gen_checkpoint is required (a local HiFi-GAN generator checkpoint with weight norm intact)')
        if disc_checkpoint is None:
            raise ValueError('HiFiGanFineTuner: disc_checkpoint is required (a local do_* checkpoint or its dict): this package has no '
                             'initialiser for the discriminators')
        self.device = torch.device(device)
        state = _checkpoint_state(gen_checkpoint)
        self.generator = HiFiGANGenerator(config_from_state(state) if config is None else config)
        self.generator.load_state_dict(state, strict=True)
        self.generator.to(self.device).train()
        ckpt = _checkpoint(disc_checkpoint)
        self.discriminators = HiFiGanDiscriminators(ckpt, self.device)
        self.lr_decay, self.power_iterations = float(lr_decay), int(power_iterations)
        betas = (adam_b1, adam_b2)
        D = self.discriminators
        self.optim_g = NormedAdamW(_layers('', self.generator), learning_rate, betas, leaves=True)
        msd_first = [layer for tag, module in reversed(D.named()) for layer in _layers(tag + '.', module)]         # as line 134
        self.optim_d = NormedAdamW(msd_first, learning_rate, betas)
        self.step, self.epoch = 0, 0
        if not reset_optimizers and 'optim_g' in ckpt and 'optim_d' in ckpt:
            self.optim_g.load_state_dict(ckpt['optim_g'])
            self.optim_d.load_state_dict(ckpt['optim_d'])
            self.step, self.epoch = int(ckpt.get('steps', 0)), int(ckpt.get('epoch', 0))
            for opt in (self.optim_g, self.optim_d):
                opt.lr = _decayed(opt.initial_lr, self.lr_decay, self.epoch)
        self.mel_l1 = MelL1Loss(fmax=None, device=self.device)
        self._refresh_discriminators()

    def _refresh_discriminators(self):
        """The discriminators' packs from the optimiser's W (the spectral-normed sub-discriminator folds its own parameters)."""
        self.discriminators.refresh_weights(self.optim_d.folded())

    def discriminator_gradients(self, y, y_hat):
        """-> ({loss_disc_f, loss_disc_s}, the gradients as ``optim_d.step`` takes them) of ``discriminator_loss_grad(folded=True)``."""
        two, grads = self.discriminators.discriminator_loss_grad(y, y_hat, power_iterations=self.power_iterations, folded=True)
        return two, {f'{tag}.{k}': g for tag in grads for k, g in grads[tag].items()}

    def generator_gradients(self):
        """-> the gradients as ``optim_g.step`` takes them, read off the folded leaves and the biases after ``backward()``."""
        return {name: (W.grad, b.grad) for name, (W, b) in self.optim_g.folded().items()}

    def forward_backward(self, x, y, y_mel, lengths=None):
        """``train_step`` up to, and without, ``optim_g.step``: the discriminators ARE stepped.  -> (the seven losses as a device vector,
        the generator's gradients)."""
        if y.dim() == 2:
            y = y[:, None, :]
        B, _, T = x.shape
        frames = [T] * B if lengths is None else [int(v) for v in lengths]
        self.optim_g.zero_grad()
        y_g_hat = generator_forward_folded(self.generator, x, self.optim_g.folded(), frames)
        loss_mel = self.mel_l1(y_g_hat[:, 0], [HOP * f for f in frames], y_mel)
        two, grads = self.discriminator_gradients(y, y_g_hat.detach())
        self.optim_d.step(grads)
        self._refresh_discriminators()
        adv = self.discriminators.generator_losses(y, y_g_hat)
        loss_gen_all = adv['loss_gen_s'] + adv['loss_gen_f'] + adv['loss_fm_s'] + adv['loss_fm_f'] + loss_mel
        loss_gen_all.backward()
        seven = dict(two, **adv, loss_mel=loss_mel)
        return torch.stack([seven[k].detach().float() for k in LOSS_NAMES]), self.generator_gradients()

    def train_step(self, x, y, y_mel, lengths=None) -> StepLosses:
        """x (B, 80, T) mel, y (B, 256 T) or (B, 1, 256 T), y_mel (B, 80, T) the full-band mel of y; ``lengths``: frames per row (host
        ints) or None.  -> the seven losses; no host synchronisation unless they are read."""
        losses, grads = self.forward_backward(x, y, y_mel, lengths)
        self.optim_g.step(grads)
        self.generator._inference = None             # a raw kernel write bumps no version counter: drop the no-grad path's cached weights
        self.step += 1
        return StepLosses(losses)

    def end_epoch(self):
        """Lines 311-312: both learning rates x lr_decay."""
        self.epoch += 1
        for opt in (self.optim_g, self.optim_d):
            opt.lr = opt.lr * self.lr_decay

    def validate(self, batches) -> float:
        """Lines 273-302: the mean over ``(x, y_mel)`` pairs of ``F.l1_loss(y_mel, mel(generator(x)))``, under no_grad."""
        total, n = 0.0, 0
        with torch.no_grad():
            for x, y_mel in batches:
                wav = self.generator(x.to(self.device))[:, 0]
                mel, _, _ = self.mel_l1.frontend(wav, [wav.shape[1]] * wav.shape[0])
                total += torch.nn.functional.l1_loss(y_mel.to(self.device), mel).item()
                n += 1
        return total / n if n else 0.0

    def save_checkpoint(self, output_dir, save_disc=False):
        """Lines 88-107: ``g_{step:08d}`` = {'generator': state dict, weight norm intact}; with ``save_disc`` ``do_{step:08d}`` = {'mpd',
        'msd', 'optim_g', 'optim_d', 'steps', 'epoch'}.  -> the paths written."""
        os.makedirs(output_dir, exist_ok=True)
        cpu = lambda sd: {k: v.detach().cpu() for k, v in sd.items()}
        paths = [os.path.join(output_dir, f'g_{self.step:08d}')]
        torch.save({'generator': cpu(self.generator.state_dict())}, paths[0])
        if save_disc:
            D = self.discriminators
            optim = lambda o: {'state': {i: cpu(s) for i, s in o['state'].items()}, 'param_groups': o['param_groups']}
            paths.append(os.path.join(output_dir, f'do_{self.step:08d}'))
            torch.save({'mpd': cpu(D.mpd.state_dict()), 'msd': cpu(D.msd.state_dict()), 'optim_g': optim(self.optim_g.state_dict()),
                        'optim_d': optim(self.optim_d.state_dict()), 'steps': self.step, 'epoch': self.epoch}, paths[1])
        return paths

    def fit(self, data, training_steps, output_dir=None, validation_interval=1000, checkpoint_interval=1000, save_disc=False,
            log=None) -> FitResult:
        """Lines 196-319 around ``train_step``: until ``step`` reaches ``training_steps``, one step on ``data.batch(step)``
        (vocoder_data.HiFiGanFineTuneData: a function of ``(seed, step)``, nothing crosses the host); ``end_epoch()`` when the step count
        reaches a multiple of ``data.steps_per_epoch``; ``validate(data.val_batches())`` every ``validation_interval`` steps; with an
        ``output_dir``, ``save_checkpoint`` every ``checkpoint_interval`` steps and at the end.  ``log(step, StepLosses)`` is called
        after every step; the losses cross to the host only if it reads them.  A 0 interval turns its action off.

        ``epoch`` counts completed passes in every checkpoint written here: at a pass boundary ``end_epoch()`` comes first, and a
        partial last pass is closed (the reference steps its schedulers after the ``break`` too) only AFTER the final checkpoint.  So
        a new tuner made from the files of ``fit(k)`` and run to ``N`` with the same ``data`` is bitwise the tuner of ``fit(N)``.  A
        checkpoint saved by hand after a ``fit`` that ended mid-pass already counts that pass, and does not resume exactly."""
        per_pass = int(data.steps_per_epoch)
        ran, losses, validation, saved = 0, None, {}, None
        while self.step < training_steps:
            losses = self.train_step(*data.batch(self.step)[:3])
            ran += 1
            if log is not None:
                log(self.step, losses)
            if self.step % per_pass == 0:
                self.end_epoch()
            if validation_interval and self.step % validation_interval == 0:
                validation[self.step] = self.validate(data.val_batches())
            if output_dir is not None and checkpoint_interval and self.step % checkpoint_interval == 0:
                self.save_checkpoint(output_dir, save_disc)
                saved = self.step
        if output_dir is not None and saved != self.step:
            self.save_checkpoint(output_dir, save_disc)
        if ran and self.step % per_pass:
            self.end_epoch()
        return FitResult(ran, losses, validation)


__all__ = ['HiFiGanFineTuner', 'StepLosses', 'FitResult', 'LOSS_NAMES']
