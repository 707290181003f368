"""HiFi-GAN discriminators on gfx950 (reference src/daft_exprt/vocoder/discriminators.py): the forward, the GAN losses, the
backward of the generator-side losses to the generated waveform, and the discriminator step (loss_disc to every parameter).

``MultiPeriodDiscriminator`` / ``DiscriminatorP`` and ``MultiScaleDiscriminator`` / ``DiscriminatorS`` own exactly the reference's
state-dict keys and shapes (90 and 80 tensors), so ``load_state_dict(strict=True)`` takes the ``['mpd']`` / ``['msd']`` entries of a
reference ``do_*`` checkpoint.  ``forward(y, y_hat)`` returns ``(y_d_rs, y_d_gs, fmap_rs, fmap_gs)`` as the reference does; every layer
runs in csrc/dx_disc.hip (there is no PyTorch fallback and no CPU path), real and generated audio as one batch of 2B rows, one launch
per layer.  The feature maps are permuted VIEWS of the kernels' channels-last buffers ((B, C, H, p) and (B, C, N)), not copies.

Stated once (*One layer table*): ``layer_table`` holds a sub-discriminator's layers at one input length, and the forward, both
backwards and the workspace query walk it; a pass lists its eight sub-discriminators once (``_Sub``), and the losses, both backwards and
the MSD's pooled chain follow that list.  tests/test_discriminators_launches_cpu.py holds every library call to a recorded sequence.

Weight folding, once and lazily (``refresh_weights()`` drops the folded copies; ``load_state_dict`` calls it):
  * weight norm (``weight_g`` / ``weight_v``): ``torch._weight_norm(v, g, 0)``;
  * spectral norm (the first MSD sub-discriminator: ``weight_orig`` / ``weight_u`` / ``weight_v``; told apart by ``weight_orig``):
    EVAL-mode semantics, ``W = weight_orig / (u . (W_mat v))`` with the stored ``u`` and ``v``.  ``.train()`` does not change the
    forward; the reference's train-mode power iteration runs only where it is asked for, ``discriminator_loss_grad(...,
    power_iterations=n)``.

``forward``, ``losses`` and the three loss functions have no backward: with grad mode on, an input (or a parameter of the module) that
requires grad raises instead of returning a silently detached result.  The parameters are created with ``requires_grad=False``.
Two backwards exist, both on ``HiFiGanDiscriminators``, neither through the parameters' autograd:
  * ``generator_losses`` / ``generator_loss_grad`` (csrc/dx_disc_bwd.hip): the gradient of loss_gen and loss_fm of both
    discriminators with respect to ``y_hat`` only; ``y`` and the weights are constants;
  * ``discriminator_loss_grad`` / ``discriminator_backward`` (csrc/dx_disc_wgrad.hip, f32 only): the gradient of loss_disc_f and
    loss_disc_s with respect to every ``nn.Parameter`` of both discriminators, returned as tensors or added into ``.grad``; both
    waveforms are constants and the parameters stay frozen leaves.

``discriminator_loss``, ``generator_loss`` and ``feature_loss`` keep the reference signatures and run through ``dx_disc_losses``.
The one deviation: the per-sub-discriminator entries are 0-d device tensors where the reference returns ``.item()`` floats (no host
synchronisation happens here).  ``HiFiGanDiscriminators.losses`` computes the six totals of finetune_hifigan.py:218-241 in one call.
"""
from __future__ import annotations

import functools
import os
from collections import namedtuple

import torch
from torch import nn

from ._lib import lib, packed as _packed, stream as _stream

LRELU_SLOPE = 0.1
PERIODS = (2, 3, 5, 7, 11)
PRECISIONS = {'f32': 0, 'bf16': 1}
# (Cin, Cout, taps, stride, groups, padding)
MPD_LAYERS = ((1, 32, 5, 3, 1, 2), (32, 128, 5, 3, 1, 2), (128, 512, 5, 3, 1, 2), (512, 1024, 5, 3, 1, 2), (1024, 1024, 5, 1, 1, 2))
MSD_LAYERS = ((1, 128, 15, 1, 1, 7), (128, 128, 41, 2, 4, 20), (128, 256, 41, 2, 16, 20), (256, 512, 41, 4, 16, 20),
              (512, 1024, 41, 4, 16, 20), (1024, 1024, 41, 1, 16, 20), (1024, 1024, 5, 1, 1, 2))
POST = (1024, 1, 3, 1, 1, 1)
LOSS_NAMES = ('loss_disc_f', 'loss_gen_f', 'loss_fm_f', 'loss_disc_s', 'loss_gen_s', 'loss_fm_s')
GEN_LOSS_NAMES = ('loss_gen_f', 'loss_fm_f', 'loss_gen_s', 'loss_fm_s')     # the generator-side losses: the ones with a backward


def conv_out(n, taps, stride, pad):
    return (n + 2 * pad - taps) // stride + 1


class Layer(namedtuple('Layer', 'name cin cout taps stride groups pad n_in n_out p')):
    """One convolution of a sub-discriminator at one input length; ``name``: 'convs.<i>' or 'conv_post', the module's name in it.  Its
    maps are channels-last, (rows, n, p, c): ``n_in`` positions of ``cin`` channels in, ``n_out`` of ``cout`` out, ``p`` columns per
    position (the period; 1: no folding)."""

    def strides(self, side):
        """-> (batch stride, column stride, position stride) in elements of the layer's input ('in') or output ('out') map, as the
        kernels take them: a kernel row is one column of one batch row."""
        n, c = (self.n_in, self.cin) if side == 'in' else (self.n_out, self.cout)
        return n * self.p * c, c, self.p * c


@functools.lru_cache(maxsize=None)
def layer_table(layers, T=1, p=1):
    """The layers of one sub-discriminator (``MPD_LAYERS`` / ``MSD_LAYERS``, then ``POST``) on T samples folded by period p -> a tuple
    of ``Layer``.  Host only; every walk over the layers (forward, both backwards, the workspace query) runs from this.  Only n_in and
    n_out depend on T and p: where the names and shapes are all that is read, the defaults serve."""
    table, n = [], -(-T // p)
    for i, (cin, cout, taps, stride, groups, pad) in enumerate(layers + (POST,)):
        name = f'convs.{i}' if i < len(layers) else 'conv_post'
        table.append(Layer(name, cin, cout, taps, stride, groups, pad, n, conv_out(n, taps, stride, pad), p))
        n = table[-1].n_out
    return tuple(table)


def _halves(t):
    """-> the device addresses of the real and the generated half of a (2B, ...) fp32 buffer."""
    return t.data_ptr(), t.data_ptr() + 4 * (t.numel() // 2)


def _frozen(t):
    return nn.Parameter(t, requires_grad=False)


class _WNConv(nn.Module):
    """Parameters of one weight-normed convolution, named as torch.nn.utils.weight_norm names them."""

    def __init__(self, w_shape):
        super().__init__()
        self.bias = _frozen(torch.zeros(w_shape[0]))
        self.weight_g = _frozen(torch.ones(w_shape[0], *([1] * (len(w_shape) - 1))))
        self.weight_v = _frozen(torch.zeros(*w_shape))


class _SNConv(nn.Module):
    """Parameters and buffers of one spectral-normed convolution, named as torch.nn.utils.spectral_norm names them."""

    def __init__(self, w_shape):
        super().__init__()
        cols = 1
        for s in w_shape[1:]:
            cols *= s
        self.bias = _frozen(torch.zeros(w_shape[0]))
        self.weight_orig = _frozen(torch.zeros(*w_shape))
        self.register_buffer('weight_u', torch.zeros(w_shape[0]))
        self.register_buffer('weight_v', torch.zeros(cols))


def fold_weight(state: dict, name: str) -> torch.Tensor:
    """The convolution weight of layer ``name`` of a discriminator state dict: folded weight norm, or eval-mode spectral norm."""
    if name + '.weight_orig' in state:
        w = state[name + '.weight_orig'].float()
        u, v = state[name + '.weight_u'].float(), state[name + '.weight_v'].float()
        sigma = torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
        return w / sigma
    if name + '.weight_v' in state and name + '.weight_g' in state:
        return torch._weight_norm(state[name + '.weight_v'].float(), state[name + '.weight_g'].float(), 0)
    raise KeyError(f'discriminator state dict has no weight for {name!r}')


def layer_names(state: dict):
    return [k[:-len('.bias')] for k in state if k.endswith('.bias')]


def fold_state_dict(state: dict) -> dict:
    """-> {layer: (weight, bias)}, fp32, on the tensors' own device."""
    return {n: (fold_weight(state, n).detach().contiguous(), state[n + '.bias'].float().detach().contiguous()) for n in layer_names(state)}


def _below(named, prefix):
    """The entries of ``named`` whose key starts with ``prefix``, keyed by the rest; None if ``named`` is None or holds none."""
    if named is None:
        return None
    return {k[len(prefix):]: v for k, v in named.items() if k.startswith(prefix)} or None


def _check_inputs(*xs):
    x = xs[0]
    for t in xs:
        if not torch.is_tensor(t) or t.dim() != 3 or t.shape[1] != 1 or t.shape[2] < 1 or t.shape[0] < 1:
            raise ValueError(f'the discriminators take (B, 1, T) waveforms, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}')
        if t.shape != x.shape or t.device != x.device:
            raise ValueError(f'y and y_hat must agree in shape and device, got {tuple(x.shape)} on {x.device} and {tuple(t.shape)} on {t.device}')
        if t.dtype != torch.float32:
            raise ValueError(f'the discriminators take fp32 waveforms, got {t.dtype}')


def _check_reflect(T, periods):
    for p in periods:
        if T % p and p - T % p >= T:
            raise ValueError(f'period {p}: the reflect padding ({p - T % p} samples) must be shorter than the signal ({T} samples)')


def _require_gpu(device, what='the HiFi-GAN discriminators run on the GPU (gfx950 HIP kernels)'):
    if device.type != 'cuda':
        raise RuntimeError(what + '; there is no CPU path')


def _require_frozen(modules, message, inputs=()):
    """No parameter of ``modules`` (and none of ``inputs``) may require grad."""
    if any(t.requires_grad for t in inputs) or any(q.requires_grad for m in modules for q in m.parameters()):
        raise RuntimeError(message)


def _check_run(module, *xs):
    """The guards of the forward-only entry points."""
    if torch.is_grad_enabled():
        _require_frozen((module,), 'the discriminators are forward only: their backward is not built, and an input or parameter requires grad '
                                   '(run under torch.no_grad() or detach the input)', xs)
    _require_gpu(xs[0].device)


def _check_forward(owner, y, y_hat):
    """The guards of ``HiFiGanDiscriminators.losses``: forward only, as ``MultiPeriodDiscriminator.forward``."""
    _check_run(owner.mpd, y, y_hat)


def _check_differentiable(owner, y, y_hat):
    """The guards of the entry points that have a backward: only ``y_hat`` may require grad."""
    if y.requires_grad:
        raise RuntimeError('the discriminators\' backward goes to y_hat only: y must not require grad')
    _require_frozen((owner.mpd, owner.msd), 'the discriminators\' backward goes to y_hat only: their parameters are constants and must not require grad')
    _require_gpu(y.device)


def _check_train(owner, y, y_hat):
    """The guards of the discriminator step: the parameters stay frozen leaves (their gradients are returned, or added to ``.grad``)."""
    if owner.precision != 'f32':
        raise RuntimeError(f"HiFiGanDiscriminators: gradients exist for precision 'f32' only, got {owner.precision!r}")
    _require_frozen((owner.mpd, owner.msd), 'the discriminator step keeps the parameters frozen (requires_grad=False) and hands their gradients '
                                            'out itself: a parameter requires grad')
    _require_gpu(y.device)


def _check_power_iterations(n):
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f'power_iterations must be a non-negative integer, got {n!r}')
    return n


def power_iterate(weight, u, v, n, eps=1e-12):
    """``n`` steps of torch.nn.utils.spectral_norm's train-mode power iteration on ``weight`` (Cout, ...), IN PLACE on ``u`` (Cout) and
    ``v`` (the rest): v <- normalize(W^T u), u <- normalize(W v), W = weight as a (Cout, -1) matrix.  ``n = 0`` touches nothing.
    -> sigma = u . (W v), 0-d.  Any device; no gradient."""
    with torch.no_grad():
        w = weight.detach().reshape(weight.shape[0], -1)
        for _ in range(_check_power_iterations(n)):
            torch.nn.functional.normalize(torch.mv(w.t(), u), dim=0, eps=eps, out=v)
            torch.nn.functional.normalize(torch.mv(w, v), dim=0, eps=eps, out=u)
        return torch.dot(u, torch.mv(w, v))


def _norm_backward(conv, name, dw, db, out):
    """The folded pair's gradient (dw in the kernels' (Cout, Cin / groups, taps), db) -> the gradients of ``conv``'s own parameters,
    into ``out`` under the state-dict keys: torch's backward of the weight norm, or of W / sigma with u and v constants."""
    out[name + '.bias'] = db
    with torch.enable_grad():
        if isinstance(conv, _SNConv):
            w0 = conv.weight_orig.detach().requires_grad_(True)
            sigma = torch.dot(conv.weight_u, torch.mv(w0.reshape(w0.shape[0], -1), conv.weight_v))
            w = w0 / sigma
            out[name + '.weight_orig'], = torch.autograd.grad(w, (w0,), dw.view_as(w))
        else:
            g, v = conv.weight_g.detach().requires_grad_(True), conv.weight_v.detach().requires_grad_(True)
            w = torch._weight_norm(v, g, 0)
            out[name + '.weight_g'], out[name + '.weight_v'] = torch.autograd.grad(w, (g, v), dw.view_as(w))


class _Arena:
    """Hands out the same buffers, in the same order, on every pass (``reset()`` starts a pass)."""

    def __init__(self):
        self.bufs, self.i = [], 0

    def reset(self):
        self.i = 0

    def __call__(self, shape, device):
        if self.i == len(self.bufs):
            self.bufs.append(torch.empty(shape, dtype=torch.float32, device=device))
        t = self.bufs[self.i]
        assert tuple(t.shape) == tuple(shape)
        self.i += 1
        return t


def _fresh(shape, device):
    return torch.empty(shape, dtype=torch.float32, device=device)


# One sub-discriminator of one pass over real + generated rows.  module: 'discriminators.<index>' of the 'mpd' / 'msd' (tag); set_id: 0
# MPD, 1 MSD, the set of its loss rows: it reads slots 2 set_id (gen) and 2 set_id + 1 (fm) of the four generator-side upstream weights,
# slot set_id of the two discriminator-side ones; level: its input x (2B, T_level) is the waveforms pooled that often; table: layer_table
# of the module at T_level; score (2B, N, p); maps: the channels-last feature maps (2B, N_i, p, C_i) of convs.<i>
_Sub = namedtuple('_Sub', 'module tag index set_id level x table score maps')


class _SubDiscriminator(nn.Module):
    LAYERS = ()
    period = 1

    def _init_layers(self, conv_cls, two_d, precision):
        if precision not in PRECISIONS:
            raise ValueError(f'precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        self.precision = precision
        tail = (1,) if two_d else ()
        self.convs = nn.ModuleList([conv_cls((cout, cin // g, k) + tail) for cin, cout, k, _, g, _ in self.LAYERS])
        self.conv_post = conv_cls((POST[1], POST[0], POST[2]) + tail)
        self._drop_weights()

    def _drop_weights(self, folded=None):
        """Everything derived from the weights: the forward's packs, the backward's, and the folded pairs handed in from outside."""
        self._packs = None
        self._dgrad = None
        self._folded = folded

    def refresh_weights(self, folded=None):
        """Drop the folded, packed device weights: the next forward folds the current parameters again.  ``folded``: {layer: (W, bias)}
        that the caller vouches to BE the fold of the current parameters (vocoder_optim.NormedAdamW.folded(): the optimiser kernel
        writes W as it steps g and v); the next packs are built from these tensors instead of folding with torch.  They are dropped
        again by any ``load_state_dict``, ``.to()`` or plain ``refresh_weights()``."""
        if folded is not None:
            names = [ly.name for ly in layer_table(self.LAYERS)]
            if sorted(folded) != sorted(names):
                raise ValueError(f'refresh_weights: folded must hold exactly the layers {names}, got {sorted(folded)}')
            for n in names:
                w, v = folded[n][0], self.get_submodule(n).weight_v
                if w.numel() != v.numel() or w.device != v.device or w.dtype != torch.float32 or not w.is_contiguous():
                    raise ValueError(f'refresh_weights: the folded weight of {n} must be contiguous fp32 with weight_v\'s {v.numel()} elements on {v.device}')
        self._drop_weights(folded)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._drop_weights()
        return out

    def _apply(self, fn, *args, **kwargs):
        self._drop_weights()                    # .to() / .cuda(): the packs follow the parameters
        return super()._apply(fn, *args, **kwargs)

    def folded(self) -> dict:
        """-> {layer: (weight (Cout, Cin / groups, taps), bias)} on the parameters' device."""
        if self._folded is not None:             # handed in by refresh_weights(folded): views, no fold here
            return {n: (w.detach().view(w.shape[0], w.shape[1], w.shape[2]), b.detach()) for n, (w, b) in self._folded.items()}
        out = fold_state_dict({k: v.detach() for k, v in self.state_dict().items()})
        return {n: (w.reshape(w.shape[0], w.shape[1], w.shape[2]).contiguous(), b) for n, (w, b) in out.items()}

    def _device_weights(self):
        """{layer: (weight, bias)}: the folded pair of the first and the last layer, the operand pack of every layer between."""
        if self._packs is None:
            bf16, dev, P = PRECISIONS[self.precision], self.conv_post.bias.device, self.folded()
            for ly in layer_table(self.LAYERS)[1:-1]:
                w, b = P[ly.name]
                P[ly.name] = (_packed('disc', w, (ly.cout, ly.cin // ly.groups, ly.taps, bf16), dev), b)
            self._packs = P
        return self._packs

    def _dgrad_weights(self):
        """{layer: the transposed, per-stride-phase pack of dx_disc_conv_dgrad}, built on the first backward only."""
        if self._dgrad is None:
            bf16, dev, F = PRECISIONS[self.precision], self.conv_post.bias.device, self.folded()
            self._dgrad = {ly.name: _packed('disc_dgrad', F[ly.name][0], (ly.cin, ly.cout, ly.groups, ly.taps, ly.stride, bf16), dev)
                           for ly in layer_table(self.LAYERS)[1:-1]}
        return self._dgrad

    def forward(self, x):
        """x (B, 1, T) -> (scores (B, n), [feature maps: 6 of (B, C, H, p), or 8 of (B, C, N)])."""
        _check_inputs(x)
        _check_reflect(x.shape[2], (self.period,))
        _check_run(self, x)
        return self._views(*self._run(x.reshape(x.shape[0], -1).contiguous(), _fresh))

    def _run(self, x2, alloc):
        """x2 (R, T) fp32 contiguous on the device -> (scores (R, N, p), [channels-last feature maps (R, N_i, p, C_i)]): one launch per
        layer."""
        L, st, bf16 = lib(), _stream(x2.device), PRECISIONS[self.precision]
        P = self._device_weights()
        (R, T), p, dev = x2.shape, self.period, x2.device
        first, *hidden, post = layer_table(self.LAYERS, T, p)
        w, b = P[first.name]
        cur = alloc((R, first.n_out, p, first.cout), dev)
        L.dx_disc_first(x2.data_ptr(), T, T, w.data_ptr(), b.data_ptr(), cur.data_ptr(), R, p, first.cout, first.taps, first.stride, first.pad, st)
        maps = [cur]
        for ly in hidden:
            w, b = P[ly.name]
            out = alloc((R, ly.n_out, p, ly.cout), dev)
            L.dx_disc_conv(cur.data_ptr(), *ly.strides('in'), w.data_ptr(), b.data_ptr(), out.data_ptr(), *ly.strides('out'), R * p, p, ly.n_in,
                           ly.cin, ly.cout, ly.groups, ly.taps, ly.stride, ly.pad, 1, bf16, st)
            maps.append(out)
            cur = out
        w, b = P[post.name]
        score = alloc((R, post.n_out, p), dev)
        L.dx_disc_post(cur.data_ptr(), *post.strides('in'), w.data_ptr(), b.data_ptr(), score.data_ptr(), *post.strides('out'), R * p, p,
                       post.n_in, post.cin, post.taps, st)
        return score, maps

    def _run_bwd(self, sub, gw, dz, dy, accumulate):
        """The chain of one sub-discriminator of a pass from its scores down to its input: gw the four upstream gradients (device); dz
        two buffers for the pre-activation gradients; dy (B, T_level) receives (accumulate: is added) the gradient of the generated
        rows.  One launch per layer."""
        L, st, bf16 = lib(), _stream(sub.score.device), PRECISIONS[self.precision]
        P, D = self._device_weights(), self._dgrad_weights()
        gen, fm = gw.data_ptr() + 4 * (2 * sub.set_id), gw.data_ptr() + 4 * (2 * sub.set_id + 1)
        B, p = dy.shape[0], self.period
        first, *hidden, post = sub.table
        last = sub.maps[-1]
        (sr, sg), (r, g) = _halves(sub.score), _halves(last)
        cur, nxt = dz
        L.dx_disc_post_bwd(sr, sg, *post.strides('out'), P[post.name][0].data_ptr(), cur.data_ptr(), r, g, *post.strides('in'), gen, fm,
                           2.0 / (sub.score.numel() // 2), 2.0 / (last.numel() // 2), B * p, p, post.n_in, post.cin, post.taps, 1, st)
        for ly, below in zip(reversed(hidden), reversed(sub.maps[:-1])):
            r, g = _halves(below)
            L.dx_disc_conv_dgrad(cur.data_ptr(), *ly.strides('out'), D[ly.name].data_ptr(), nxt.data_ptr(), r, g, *ly.strides('in'), fm,
                                 2.0 / (below.numel() // 2), B * p, p, ly.n_in, ly.cin, ly.cout, ly.groups, ly.taps, ly.stride, ly.pad, 1, bf16, st)
            cur, nxt = nxt, cur
        L.dx_disc_first_bwd(cur.data_ptr(), P[first.name][0].data_ptr(), dy.data_ptr(), dy.shape[1], dy.shape[1], B, p, first.cout, first.taps,
                            first.stride, first.pad, int(accumulate), st)

    def _wgrad_workspace(self, sub):
        """-> bytes of the largest workspace the weight-gradient kernels ask for on this sub-discriminator of a pass."""
        L, nb, p, (R, T) = lib(), torch.zeros(1, dtype=torch.long), self.period, sub.x.shape
        first, *hidden, post = sub.table
        L.dx_disc_first_wgrad_size(R, T, p, first.cout, first.taps, first.stride, first.pad, nb.data_ptr())
        need = int(nb.item())
        for ly in hidden:
            L.dx_disc_wgrad_size(R * p, ly.n_in, ly.cin, ly.cout, ly.groups, ly.taps, ly.stride, ly.pad, nb.data_ptr(), None)
            need = max(need, int(nb.item()))
        L.dx_disc_post_wgrad_size(R * p, post.n_in, post.cin, post.taps, nb.data_ptr())
        return max(need, int(nb.item()))

    def _run_wgrad(self, sub, gw, dz, ws, zero):
        """The discriminator step of one sub-discriminator of a pass (csrc/dx_disc_wgrad.hip), real rows first; gw -> ONE device float,
        the upstream gradient of its discriminator loss; dz two buffers for the pre-activation gradients of all 2B rows; ws the
        workspace; zero -> a device zero (dx_disc_conv_dgrad's feature-matching weight) -> {layer: (dW (Cout, Cin / groups, taps), db)}
        of the folded pairs.  Top down, each layer's weight gradient launched before its data gradient, so the two dz buffers suffice."""
        L, st, dev = lib(), _stream(sub.score.device), sub.score.device
        P, D = self._device_weights(), self._dgrad_weights()
        (R, T), p = sub.x.shape, self.period
        first, *hidden, post = sub.table
        cur, nxt = dz
        out = {}
        dW, db = _fresh((post.cout, post.cin, post.taps), dev), _fresh((post.cout,), dev)
        L.dx_disc_post_wgrad(sub.score.data_ptr(), *post.strides('out'), P[post.name][0].data_ptr(), sub.maps[-1].data_ptr(), cur.data_ptr(),
                             *post.strides('in'), gw, 2.0 / (sub.score.numel() // 2), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                             R * p, R // 2 * p, p, post.n_in, post.cin, post.taps, st)
        out[post.name] = (dW, db)
        for ly, below in zip(reversed(hidden), reversed(sub.maps[:-1])):
            dW, db = _fresh((ly.cout, ly.cin // ly.groups, ly.taps), dev), _fresh((ly.cout,), dev)
            L.dx_disc_wgrad(below.data_ptr(), *ly.strides('in'), cur.data_ptr(), *ly.strides('out'), dW.data_ptr(), db.data_ptr(), ws.data_ptr(),
                            ws.numel(), R * p, p, ly.n_in, ly.cin, ly.cout, ly.groups, ly.taps, ly.stride, ly.pad, st)
            out[ly.name] = (dW, db)
            L.dx_disc_conv_dgrad(cur.data_ptr(), *ly.strides('out'), D[ly.name].data_ptr(), nxt.data_ptr(), below.data_ptr(), below.data_ptr(),
                                 *ly.strides('in'), zero, 0.0, R * p, p, ly.n_in, ly.cin, ly.cout, ly.groups, ly.taps, ly.stride, ly.pad, 1, 0, st)
            cur, nxt = nxt, cur
        dW, db = _fresh((first.cout, 1, first.taps), dev), _fresh((first.cout,), dev)
        L.dx_disc_first_wgrad(sub.x.data_ptr(), T, T, cur.data_ptr(), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), R, p,
                              first.cout, first.taps, first.stride, first.pad, st)
        out[first.name] = (dW, db)
        return out


class DiscriminatorP(_SubDiscriminator):
    """One period sub-discriminator (discriminators.py:28-66): (5, 1) convolutions over the period-folded signal."""
    LAYERS = MPD_LAYERS

    def __init__(self, period, precision='f32'):
        super().__init__()
        self.period = int(period)
        self._init_layers(_WNConv, True, precision)

    @staticmethod
    def _views(score, fmaps):
        """channels-last buffers -> the reference's (x (R, N p), [fmap (R, C, H, p)])."""
        return score.view(score.shape[0], -1), [f.permute(0, 3, 1, 2) for f in fmaps] + [score.unsqueeze(1)]


class DiscriminatorS(_SubDiscriminator):
    """One scale sub-discriminator (discriminators.py:98-124): grouped k = 41 Conv1d layers."""
    LAYERS = MSD_LAYERS

    def __init__(self, use_spectral_norm=False, precision='f32'):
        super().__init__()
        self.use_spectral_norm = bool(use_spectral_norm)
        self._init_layers(_SNConv if use_spectral_norm else _WNConv, False, precision)

    @staticmethod
    def _views(score, fmaps):
        """channels-last buffers -> the reference's (x (R, N), [fmap (R, C, N)])."""
        return score.view(score.shape[0], -1), [f.squeeze(2).permute(0, 2, 1) for f in fmaps] + [score.view(score.shape[0], 1, -1)]


class _MultiDiscriminator(nn.Module):
    POOLED = False              # each sub-discriminator after the first reads the AvgPool1d(4, 2, padding=2) of the one before

    def refresh_weights(self, folded=None):
        """``folded``: {'discriminators.<i>.<layer>': (W, bias)}, see _SubDiscriminator.refresh_weights; a sub-discriminator none of whose
        layers is named (the spectral-normed one) folds its own parameters as before."""
        for i, d in enumerate(self.discriminators):
            d.refresh_weights(_below(folded, f'discriminators.{i}.'))

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.refresh_weights()
        return out

    def forward(self, y, y_hat):
        """y, y_hat (B, 1, T) fp32 on the device -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) as the reference returns them."""
        _check_inputs(y, y_hat)
        _check_reflect(y.shape[2], [d.period for d in self.discriminators])
        _check_run(self, y, y_hat)
        B = y.shape[0]
        x2 = torch.cat([y.detach().reshape(B, -1), y_hat.detach().reshape(B, -1)], 0)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for d, (_, _, raw_score, raw_maps) in zip(self.discriminators, self._run(x2, _fresh)):
            score, fmaps = d._views(raw_score, raw_maps)
            y_d_rs.append(score[:B])
            y_d_gs.append(score[B:])
            fmap_rs.append([f[:B] for f in fmaps])
            fmap_gs.append([f[B:] for f in fmaps])
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    def _run(self, x2, alloc):
        """-> per sub-discriminator (the level of its input: how often x2 was pooled, its (R, T_level) input, scores, feature maps), the
        last two as the kernels' channels-last buffers."""
        out, level = [], 0
        for i, d in enumerate(self.discriminators):
            if i and self.POOLED:
                R, T = x2.shape
                pooled = alloc((R, T // 2 + 1), x2.device)
                lib().dx_disc_pool(x2.data_ptr(), pooled.data_ptr(), R, T, _stream(x2.device))
                x2, level = pooled, level + 1
            out.append((level, x2) + d._run(x2, alloc))
        return out


class MultiPeriodDiscriminator(_MultiDiscriminator):
    """Five period sub-discriminators, periods 2, 3, 5, 7, 11 (discriminators.py:69-91): 30 launches for both inputs."""

    def __init__(self, precision='f32'):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(p, precision) for p in PERIODS])


class MultiScaleDiscriminator(_MultiDiscriminator):
    """Three scale sub-discriminators, the first spectral-normed, the others fed through AvgPool1d(4, 2, padding=2)
    (discriminators.py:127-156): 26 launches for both inputs."""
    POOLED = True

    def __init__(self, precision='f32'):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorS(True, precision), DiscriminatorS(False, precision),
                                             DiscriminatorS(False, precision)])
        self.meanpools = nn.ModuleList([nn.Module(), nn.Module()])      # the reference's two AvgPool1d: no parameters


# ---- losses -----------------------------------------------------------------------------------------------------------------------
def _dense_pair(r, g):
    """Two equally shaped fp32 tensors -> the same element pairs as two dense blocks of memory (views where possible: a permuted view of
    a contiguous buffer is un-permuted, not copied; the means below do not depend on the element order)."""
    if r.shape != g.shape:
        raise ValueError(f'real and generated tensors differ in shape: {tuple(r.shape)} and {tuple(g.shape)}')
    r, g = r.detach(), g.detach()
    if r.dtype != torch.float32 or g.dtype != torch.float32:
        r, g = r.float(), g.float()
    if not (r.is_contiguous() and g.is_contiguous()):
        order = sorted(range(r.dim()), key=lambda d: (-r.stride(d), d))
        rp, gp = r.permute(order), g.permute(order)
        r, g = (rp, gp) if rp.is_contiguous() and gp.is_contiguous() else (r.contiguous(), g.contiguous())
    return r, g


def _loss_rows(pairs, kind, set_id):
    """-> [(r, g, code)]: each pair as dense blocks, and its code in dx_disc_losses' table."""
    rows = []
    for r, g in pairs:
        r, g = _dense_pair(r, g)
        if r.numel() == 0:
            raise ValueError('a loss over an empty tensor')
        rows.append((r, g, kind + 2 * set_id))
    return rows


class _LossPlan:
    """The device table of dx_disc_losses for a fixed list of tensors (``_loss_rows``; kept alive here), and its workspace."""

    def __init__(self, rows, n_sets, device):
        _require_gpu(device, 'the GAN losses run on the GPU (csrc/dx_disc.hip)')
        self.rows, self.n, self.n_sets = rows, len(rows), n_sets
        self.max_count, self.total = max(r.numel() for r, _, _ in rows), sum(r.numel() for r, _, _ in rows)
        self.table = torch.tensor([[r.data_ptr(), g.data_ptr(), r.numel(), code] for r, g, code in rows], dtype=torch.int64).to(device)
        nfl = torch.zeros(1, dtype=torch.long)
        lib().dx_disc_losses_workspace(self.max_count, self.n, nfl.data_ptr())
        self.partial = torch.empty(int(nfl.item()), dtype=torch.float32, device=device)
        self.device = device

    def run(self):
        """-> fp32 device vector: 3 totals per set, then 3 terms per entry."""
        out = torch.empty(3 * self.n_sets + 3 * self.n, dtype=torch.float32, device=self.device)
        lib().dx_disc_losses(self.table.data_ptr(), self.n, self.n_sets, self.max_count, self.total, self.partial.data_ptr(),
                             out.data_ptr(), _stream(self.device))
        return out


def _check_loss_inputs(tensors):
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError('the GAN losses are forward only: their backward is not built, and an input requires grad')


def discriminator_loss(disc_real_outputs, disc_generated_outputs):
    """-> (loss, r_losses, g_losses) as discriminators.py:163-174; the list entries are 0-d device tensors, not floats."""
    pairs = list(zip(disc_real_outputs, disc_generated_outputs))
    _check_loss_inputs([t for p in pairs for t in p])
    out = _LossPlan(_loss_rows(pairs, 0, 0), 1, pairs[0][0].device).run()
    return out[0], [out[3 + 3 * i] for i in range(len(pairs))], [out[3 + 3 * i + 1] for i in range(len(pairs))]


def generator_loss(disc_outputs):
    """-> (loss, gen_losses) as discriminators.py:177-185."""
    outs = list(disc_outputs)
    _check_loss_inputs(outs)
    out = _LossPlan(_loss_rows([(t, t) for t in outs], 0, 0), 1, outs[0].device).run()
    return out[1], [out[3 + 3 * i + 2] for i in range(len(outs))]


def feature_loss(fmap_r, fmap_g):
    """-> 2 x the sum over all feature maps of mean |r - g| (discriminators.py:188-194)."""
    pairs = [(rl, gl) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg)]
    _check_loss_inputs([t for p in pairs for t in p])
    return _LossPlan(_loss_rows(pairs, 1, 0), 1, pairs[0][0].device).run()[2]


def _checkpoint(checkpoint) -> dict:
    if isinstance(checkpoint, (str, os.PathLike)):
        checkpoint = torch.load(checkpoint, map_location='cpu')
    if not isinstance(checkpoint, dict) or 'mpd' not in checkpoint or 'msd' not in checkpoint:
        raise TypeError("a discriminator checkpoint is a dict with 'mpd' and 'msd' state dicts (the reference's do_* files)")
    return checkpoint


class _Plan:
    """What ``HiFiGanDiscriminators`` keeps per (B, T, device): the activation arenas of the two discriminators, the latest pass over
    them, the loss table, the workspaces of the two backwards (made on first use) and the upstream weights uploaded so far."""

    def __init__(self):
        self.arenas = {'mpd': _Arena(), 'msd': _Arena()}
        self.passes, self.subs = 0, []           # the passes begun so far; the sub-discriminators of the latest one
        self.loss = None                         # _LossPlan over the arenas' buffers
        self.bwd = None                          # (dz pair, [gradient buffer of each pooled input])
        self.train = None                        # (dz pair, workspace, device zero)
        self.uploaded = {}

    def begin(self):
        """Starts a pass: the arenas hand out their buffers from the first again."""
        self.passes += 1
        for arena in self.arenas.values():
            arena.reset()

    def check_current(self, stamp):
        if self.passes != stamp:
            raise RuntimeError('the discriminators\' feature maps of this pass were overwritten by a later pass at the same (B, T): '
                               'call backward() before the next losses() / generator_losses() / generator_loss_grad() at that shape')

    def upstream(self, weights, n, device):
        """``weights``: n floats or an fp32 tensor of n on ``device`` -> an fp32 device tensor of n, read by the kernels.  Floats are
        uploaded once per plan: a captured graph must not copy from host memory."""
        held = torch.is_tensor(weights)
        key = None if held else tuple(float(w) for w in weights)
        ok = (weights.shape == (n,) and weights.dtype == torch.float32 and weights.device == device) if held else len(key) == n
        if not ok:
            raise ValueError(f'weights: {"two" if n == 2 else "four"} floats or an fp32 tensor of {n} on the inputs\' device')
        if held:
            return weights.detach().contiguous()
        if key not in self.uploaded:
            self.uploaded[key] = torch.tensor(key, dtype=torch.float32).to(device)
        return self.uploaded[key]


class HiFiGanDiscriminators:
    """Both discriminators from a reference ``do_*`` checkpoint (a local path or its loaded dict; nothing here downloads).

    ``losses(y, y_hat)`` -> the six totals of finetune_hifigan.py:218-241 as 0-d device tensors, no host synchronisation:
    ``loss_disc_f``, ``loss_disc_s`` (discriminator_loss of the MPD / MSD scores), ``loss_gen_f``, ``loss_gen_s`` (generator_loss),
    ``loss_fm_f``, ``loss_fm_s`` (feature_loss).  56 layer launches and one ``dx_disc_losses`` call.  The activation workspace and the
    loss table are kept per (B, T), so after one eager call ``losses`` can be captured in a ``torch.cuda.graph``.
    """

    def __init__(self, checkpoint=None, device='cuda', precision='f32'):
        if checkpoint is None:
            raise ValueError('HiFiGanDiscriminators: checkpoint is required (a local do_* checkpoint or its dict); this package never downloads one')
        if precision not in PRECISIONS:
            raise ValueError(f'HiFiGanDiscriminators: precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        state = _checkpoint(checkpoint)
        self.precision = precision
        self.device = torch.device(device)
        self.mpd, self.msd = MultiPeriodDiscriminator(precision), MultiScaleDiscriminator(precision)
        for tag, module in self.named():
            module.load_state_dict(state[tag], strict=True)
            module.to(self.device).eval()
        self._plans = {}

    def named(self):
        """-> (('mpd', the MPD), ('msd', the MSD)): the tags under which both discriminators' layers, folded weights and gradients are
        keyed, '<tag>.discriminators.<i>.<layer>', and the order of a pass."""
        return ('mpd', self.mpd), ('msd', self.msd)

    def refresh_weights(self, folded=None):
        """``refresh_weights`` of both discriminators; ``folded``: {'<tag>.discriminators.<i>.<layer>': (W, bias)}, as
        vocoder_optim.NormedAdamW.folded() names the layers it was given under these tags."""
        for tag, module in self.named():
            module.refresh_weights(_below(folded, tag + '.'))

    def _plan(self, y, y_hat, check):
        """The guards of an entry point (``check``: one of the three above) -> the plan of the inputs' shape."""
        _check_inputs(y, y_hat)
        _check_reflect(y.shape[2], PERIODS)
        check(self, y, y_hat)
        key = (y.shape[0], y.shape[2], y.device)
        if key not in self._plans:
            self._plans[key] = _Plan()
        return self._plans[key]

    def _pass(self, plan, y, y_hat):
        """One forward of both discriminators into the plan's arenas -> the stamp of the pass."""
        B = y.shape[0]
        plan.begin()
        x2 = torch.cat([y.detach().reshape(B, -1), y_hat.detach().reshape(B, -1)], 0)
        plan.subs = []
        for set_id, (tag, module) in enumerate(self.named()):
            for i, (d, (level, x, score, maps)) in enumerate(zip(module.discriminators, module._run(x2, plan.arenas[tag]))):
                plan.subs.append(_Sub(d, tag, i, set_id, level, x, layer_table(d.LAYERS, x.shape[1], d.period), score, maps))
        return plan.passes

    def losses(self, y, y_hat) -> dict:
        plan = self._plan(y, y_hat, _check_forward)
        self._pass(plan, y, y_hat)
        return self._losses(plan)

    def _losses(self, plan):
        if plan.loss is None:
            B = plan.subs[0].x.shape[0] // 2
            rows = []
            for set_id in range(2):
                own = [sub for sub in plan.subs if sub.set_id == set_id]
                rows += _loss_rows([(sub.score[:B], sub.score[B:]) for sub in own], 0, set_id)
                rows += _loss_rows([(f[:B], f[B:]) for sub in own for f in sub.maps + [sub.score]], 1, set_id)
            plan.loss = _LossPlan(rows, 2, plan.subs[0].x.device)
        out = plan.loss.run()
        return {name: out[i] for i, name in enumerate(LOSS_NAMES)}

    # ---- backward to the generated waveform (csrc/dx_disc_bwd.hip) -------------------------------------------------------------------
    def _forward_kept(self, y, y_hat):
        """One pass whose feature maps stay in the plan for a backward -> (plan, the pass's stamp, the four generator-side losses)."""
        plan = self._plan(y, y_hat, _check_differentiable)
        stamp = self._pass(plan, y, y_hat)
        six = self._losses(plan)
        return plan, stamp, {name: six[name] for name in GEN_LOSS_NAMES}

    def _backward(self, plan, stamp, gw):
        """gw: fp32 device tensor of 4, the upstream gradients in GEN_LOSS_NAMES order -> dy_hat (B, 1, T).  Every sub-discriminator's
        chain ends in the gradient of its own input; the pooled inputs' gradients are then folded back, last level first."""
        plan.check_current(stamp)
        dev, subs = gw.device, plan.subs
        B, T = subs[0].x.shape[0] // 2, subs[0].x.shape[1]
        if plan.bwd is None:
            biggest = max(f.numel() // 2 for sub in subs for f in sub.maps)
            lengths = {sub.level: sub.x.shape[1] for sub in subs}
            plan.bwd = (_fresh((biggest,), dev), _fresh((biggest,), dev)), [_fresh((B, lengths[k]), dev) for k in range(1, len(lengths))]
        dz, pooled = plan.bwd
        dx = [_fresh((B, T), dev)] + pooled              # per level: the gradient of that input's generated rows
        written = set()
        for sub in subs:
            sub.module._run_bwd(sub, gw, dz, dx[sub.level], sub.level in written)
            written.add(sub.level)
        L, st = lib(), _stream(dev)
        for level in range(len(dx) - 1, 0, -1):
            L.dx_disc_pool_bwd(dx[level].data_ptr(), dx[level - 1].data_ptr(), B, dx[level - 1].shape[1], 1, st)
        return dx[0].view(B, 1, T)

    def generator_losses(self, y, y_hat) -> dict:
        """-> {loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s}: the bits of ``losses()``, differentiable with respect to ``y_hat`` (only).
        The backward must run before the next pass at the same (B, T): the feature maps live in the per-shape plan."""
        out = _GeneratorLosses.apply(y_hat, self, y)
        return dict(zip(GEN_LOSS_NAMES, out))

    def generator_loss_grad(self, y, y_hat, weights=(1.0, 1.0, 1.0, 1.0)):
        """-> ({the four generator-side losses}, d sum_i weights[i] loss_i / d y_hat (B, 1, T)), without autograd.  ``weights``: four
        floats or an fp32 device tensor of 4, in the order loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s."""
        with torch.no_grad():
            plan, stamp, four = self._forward_kept(y, y_hat)
            return four, self._backward(plan, stamp, plan.upstream(weights, 4, y.device))

    # ---- the discriminator step: loss_disc to every parameter (csrc/dx_disc_wgrad.hip) ---------------------------------
    def _spectral_layers(self):
        return [c for d in self.msd.discriminators if d.use_spectral_norm for c in list(d.convs) + [d.conv_post]]

    def discriminator_loss_grad(self, y, y_hat, weights=(1.0, 1.0), power_iterations=1, folded=False):
        """-> ({'loss_disc_f', 'loss_disc_s'}, {'mpd': {state-dict key: gradient}, 'msd': {...}}): the two discriminator losses (the
        bits of ``losses()``) and the gradient of ``weights[0] loss_disc_f + weights[1] loss_disc_s`` with respect to every
        ``nn.Parameter`` of both discriminators (154 tensors, each in its parameter's own shape), without autograd.  ``weights``: two
        floats or an fp32 device tensor of 2, read on the device.  Both waveforms are constants (``y_hat`` is detached, as the reference
        passes ``y_g_hat.detach()``); the parameters stay ``requires_grad=False``.  Precision 'f32' only.

        ``power_iterations`` = n > 0 first runs n steps of the spectral norm's power iteration on the eight spectral-normed layers,
        writing ``weight_u`` / ``weight_v`` in place and dropping their folded packs (``eps`` 1e-12, as torch.nn.utils.spectral_norm);
        n = 0 is the eval-mode fold of ``forward``.  The gradient of ``weight_orig`` goes through W / sigma with u and v constants, as
        torch's.  Deviation from the reference: its train-mode ``msd(y, y_hat)`` calls the spectral sub-discriminator twice, so it
        iterates twice per step and the real and the generated rows see sigmas of successive iterations; here both halves share one
        pass and one sigma.  At the fixed point of the iteration the two agree.

        ``folded=True`` stops before torch's weight-norm backward: a weight-normed layer's entry is then the pair (dW, db) of its FOLDED
        weight (dW in the kernels' (Cout, Cin / groups, taps), weight_v's memory layout) under the key ``discriminators.<i>.<layer>``,
        which is what vocoder_optim.NormedAdamW.step takes; a spectral-normed layer's entries are unchanged.  The losses are the same
        bits either way."""
        n = _check_power_iterations(power_iterations)
        with torch.no_grad():
            plan, dev = self._plan(y, y_hat, _check_train), y.device
            gw = plan.upstream(weights, 2, dev)
            if n:
                for c in self._spectral_layers():
                    power_iterate(c.weight_orig, c.weight_u, c.weight_v, n)
                for d in self.msd.discriminators:
                    if d.use_spectral_norm:
                        d.refresh_weights()
            self._pass(plan, y, y_hat)
            six = self._losses(plan)
            subs = plan.subs
            if plan.train is None:
                biggest = max(f.numel() for sub in subs for f in sub.maps)
                need = max(sub.module._wgrad_workspace(sub) for sub in subs)
                plan.train = ((_fresh((biggest,), dev), _fresh((biggest,), dev)), torch.empty(need, dtype=torch.uint8, device=dev),
                              torch.zeros(1, dtype=torch.float32, device=dev))
            dz, ws, zero = plan.train
            grads = {tag: {} for tag, _ in self.named()}
            for sub in subs:
                pairs = sub.module._run_wgrad(sub, gw.data_ptr() + 4 * sub.set_id, dz, ws, zero.data_ptr())
                for name, (dw, db) in pairs.items():
                    conv, key = sub.module.get_submodule(name), f'discriminators.{sub.index}.{name}'
                    if folded and not isinstance(conv, _SNConv):
                        grads[sub.tag][key] = (dw, db)
                    else:
                        _norm_backward(conv, key, dw, db, grads[sub.tag])
            return {'loss_disc_f': six['loss_disc_f'], 'loss_disc_s': six['loss_disc_s']}, grads

    def discriminator_backward(self, y, y_hat, weights=(1.0, 1.0), power_iterations=1):
        """``discriminator_loss_grad`` whose gradients are ADDED into each parameter's ``.grad`` (created where it is None) -> the two
        losses.  The parameters stay frozen leaves: an optimiser steps whatever has a ``.grad``, so the discriminator step is
        ``optim_d.zero_grad(); D.discriminator_backward(y, y_hat); optim_d.step(); D.mpd.refresh_weights(); D.msd.refresh_weights()``."""
        two, grads = self.discriminator_loss_grad(y, y_hat, weights, power_iterations)
        with torch.no_grad():
            for tag, module in self.named():
                for key, q in module.named_parameters():
                    g = grads[tag][key]
                    if q.grad is None:
                        q.grad = g.clone()
                    else:
                        q.grad.add_(g)
        return two


class _GeneratorLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y_hat, owner, y):
        ctx.plan, ctx.stamp, four = owner._forward_kept(y, y_hat)
        ctx.owner = owner
        return tuple(four[name].clone() for name in GEN_LOSS_NAMES)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        ref = next(g for g in grads if g is not None)
        gw = torch.stack([torch.zeros_like(ref) if g is None else g for g in grads]).float().reshape(4).contiguous()
        return ctx.owner._backward(ctx.plan, ctx.stamp, gw), None, None


__all__ = ['DiscriminatorP', 'DiscriminatorS', 'MultiPeriodDiscriminator', 'MultiScaleDiscriminator', 'HiFiGanDiscriminators',
           'discriminator_loss', 'generator_loss', 'feature_loss']
