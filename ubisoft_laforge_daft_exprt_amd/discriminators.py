"""HiFi-GAN discriminators on gfx950 (reference src/daft_exprt/vocoder/discriminators.py): the forward, the GAN losses, the
backward of the generator-side losses to the generated waveform, and the discriminator step (loss_disc to every parameter).

``MultiPeriodDiscriminator`` / ``DiscriminatorP`` and ``MultiScaleDiscriminator`` / ``DiscriminatorS`` own exactly the reference's
state-dict keys and shapes (90 and 80 tensors), so ``load_state_dict(strict=True)`` takes the ``['mpd']`` / ``['msd']`` entries of a
reference ``do_*`` checkpoint.  ``forward(y, y_hat)`` returns ``(y_d_rs, y_d_gs, fmap_rs, fmap_gs)`` as the reference does; every layer
runs in csrc/dx_disc.hip (there is no PyTorch fallback and no CPU path), real and generated audio as one batch of 2B rows, one launch
per layer.  The feature maps are permuted VIEWS of the kernels' channels-last buffers ((B, C, H, p) and (B, C, N)), not copies.

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

import os

import torch
from torch import nn

from ._lib import lib

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


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _packed(kind, w, dims, device):
    """``dx_<kind>_pack`` of the contiguous fp32 device tensor ``w`` -> its operand pack, a uint8 device buffer of the size that
    ``dx_<kind>_pack_size`` reports; ``dims``: the arguments the two entry points share."""
    L = lib()
    nbytes = torch.zeros(1, dtype=torch.long)
    getattr(L, f'dx_{kind}_pack_size')(*dims, nbytes.data_ptr())
    buf = torch.empty(int(nbytes.item()), dtype=torch.uint8, device=device)
    getattr(L, f'dx_{kind}_pack')(w.data_ptr(), buf.data_ptr(), *dims, _stream(device))
    return buf


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


def _check_differentiable(owner, y, y_hat):
    """The guards of the entry points that have a backward: only ``y_hat`` may require grad."""
    if y.requires_grad:
        raise RuntimeError('the discriminators\' backward goes to y_hat only: y must not require grad')
    if any(q.requires_grad for m in (owner.mpd, owner.msd) for q in m.parameters()):
        raise RuntimeError('the discriminators\' backward goes to y_hat only: their parameters are constants and must not require grad')
    if y.device.type != 'cuda':
        raise RuntimeError('the HiFi-GAN discriminators run on the GPU (gfx950 HIP kernels); there is no CPU path')


def _check_train(owner, y):
    """The guards of the discriminator step: the parameters stay frozen leaves (their gradients are returned, or added to ``.grad``)."""
    if owner.precision != 'f32':
        raise RuntimeError(f"HiFiGanDiscriminators: gradients exist for precision 'f32' only, got {owner.precision!r}")
    if any(q.requires_grad for m in (owner.mpd, owner.msd) for q in m.parameters()):
        raise RuntimeError('the discriminator step keeps the parameters frozen (requires_grad=False) and hands their gradients out itself: '
                           'a parameter requires grad')
    if y.device.type != 'cuda':
        raise RuntimeError('the HiFi-GAN discriminators run on the GPU (gfx950 HIP kernels); there is no CPU path')


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


def _check_run(module, *xs):
    if torch.is_grad_enabled() and (any(t.requires_grad for t in xs) or any(q.requires_grad for q in module.parameters())):
        raise RuntimeError('the discriminators are forward only: their backward is not built, and an input or parameter requires grad '
                           '(run under torch.no_grad() or detach the input)')
    if xs[0].device.type != 'cuda':
        raise RuntimeError('the HiFi-GAN discriminators run on the GPU (gfx950 HIP kernels); there is no CPU path')


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


class _SubDiscriminator(nn.Module):
    LAYERS = ()

    def _init_layers(self, conv_cls, two_d, precision):
        if precision not in PRECISIONS:
            raise ValueError(f'precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        self.precision = precision
        tail = (1,) if two_d else ()
        self.convs = nn.ModuleList([conv_cls((cout, cin // g, k) + tail) for cin, cout, k, _, g, _ in self.LAYERS])
        self.conv_post = conv_cls((POST[1], POST[0], POST[2]) + tail)
        self._packs = None
        self._dgrad = None
        self._folded = None

    def refresh_weights(self, folded=None):
        """Drop the folded, packed device weights: the next forward folds the current parameters again.  ``folded``: {layer: (W, bias)}
        that the caller vouches to BE the fold of the current parameters (vocoder_optim.NormedAdamW.folded(): the optimiser kernel
        writes W as it steps g and v); the next packs are built from these tensors instead of folding with torch.  They are dropped
        again by any ``load_state_dict``, ``.to()`` or plain ``refresh_weights()``."""
        self._packs = None
        self._dgrad = None
        if folded is not None:
            names = [f'convs.{i}' for i in range(len(self.convs))] + ['conv_post']
            if sorted(folded) != sorted(names):
                raise ValueError(f'refresh_weights: folded must hold exactly the layers {names}, got {sorted(folded)}')
            for n in names:
                w, v = folded[n][0], (self.conv_post if n == 'conv_post' else self.convs[int(n[len('convs.'):])]).weight_v
                if w.numel() != v.numel() or w.device != v.device or w.dtype != torch.float32 or not w.is_contiguous():
                    raise ValueError(f'refresh_weights: the folded weight of {n} must be contiguous fp32 with weight_v\'s {v.numel()} elements on {v.device}')
        self._folded = folded

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.refresh_weights()
        return out

    def _apply(self, fn, *args, **kwargs):
        self._packs = None                      # .to() / .cuda(): the packs follow the parameters
        self._dgrad = None
        self._folded = None
        return super()._apply(fn, *args, **kwargs)

    def folded(self) -> dict:
        """-> {layer: (weight (Cout, Cin / groups, taps), bias)} on the parameters' device."""
        if self._folded is not None:             # handed in by refresh_weights(folded): views, no fold here
            return {n: (w.detach().view(w.shape[0], w.shape[1], w.shape[2]), b.detach()) for n, (w, b) in self._folded.items()}
        out = fold_state_dict({k: v.detach() for k, v in self.state_dict().items()})
        return {n: (w.reshape(w.shape[0], w.shape[1], w.shape[2]).contiguous(), b) for n, (w, b) in out.items()}

    def _device_weights(self):
        if self._packs is None:
            bf16 = PRECISIONS[self.precision]
            F = self.folded()
            dev = self.conv_post.bias.device
            P = {'convs.0': F['convs.0'], 'conv_post': F['conv_post']}
            for i, (cin, cout, k, _, g, _) in enumerate(self.LAYERS[1:], 1):
                w, b = F[f'convs.{i}']
                P[f'convs.{i}'] = (_packed('disc', w, (cout, cin // g, k, bf16), dev), b)
            self._packs = P
        return self._packs

    def _dgrad_weights(self):
        """The transposed, per-stride-phase packs of dx_disc_conv_dgrad, built on the first backward only."""
        if self._dgrad is None:
            bf16 = PRECISIONS[self.precision]
            F = self.folded()
            dev = self.conv_post.bias.device
            P = {}
            for i, (cin, cout, k, s, g, _) in enumerate(self.LAYERS[1:], 1):
                P[i] = _packed('disc_dgrad', F[f'convs.{i}'][0], (cin, cout, g, k, s, bf16), dev)
            self._dgrad = P
        return self._dgrad

    def _run_bwd(self, score, fmaps, B, T, p, gw, i_gen, i_fm, dz, dy, accumulate):
        """The chain of one sub-discriminator from its scores down to the waveform: score (2B, N, p) and the channels-last maps of a
        forward pass over real + generated rows; gw the four upstream gradients (device); dz two buffers for the pre-activation
        gradients; dy (B, T) receives (accumulate: is added) the gradient of the generated rows.  One launch per layer."""
        L, st, bf16 = lib(), _stream(score.device), PRECISIONS[self.precision]
        P, D = self._device_weights(), self._dgrad_weights()
        gen, fm = gw.data_ptr() + 4 * i_gen, gw.data_ptr() + 4 * i_fm
        N, C = score.shape[1], POST[0]
        last = fmaps[-1]
        (sr, sg), (r, g) = _halves(score), _halves(last)
        cur, nxt = dz
        L.dx_disc_post_bwd(sr, sg, N * p, 1, p, P['conv_post'][0].data_ptr(), cur.data_ptr(), r, g, N * p * C, C, p * C, gen, fm,
                           2.0 / (score.numel() // 2), 2.0 / (last.numel() // 2), B * p, p, N, C, POST[2], 1, st)
        for i in range(len(self.LAYERS) - 1, 0, -1):
            cin, cout, k, s, grp, pad = self.LAYERS[i]
            below = fmaps[i - 1]
            n_in, n_out = below.shape[1], fmaps[i].shape[1]
            r, g = _halves(below)
            L.dx_disc_conv_dgrad(cur.data_ptr(), n_out * p * cout, cout, p * cout, D[i].data_ptr(), nxt.data_ptr(), r, g, n_in * p * cin, cin,
                                 p * cin, fm, 2.0 / (below.numel() // 2), B * p, p, n_in, cin, cout, grp, k, s, pad, 1, bf16, st)
            cur, nxt = nxt, cur
        _, cout, k, s, _, pad = self.LAYERS[0]
        L.dx_disc_first_bwd(cur.data_ptr(), P['convs.0'][0].data_ptr(), dy.data_ptr(), dy.shape[1], T, B, p, cout, k, s, pad,
                            int(accumulate), st)

    def _wgrad_workspace(self, R, T, p):
        """-> bytes of the largest workspace the weight-gradient kernels of this sub-discriminator ask for on R rows of T samples."""
        L, nb = lib(), torch.zeros(1, dtype=torch.long)
        _, cout, k, s, _, pad = self.LAYERS[0]
        L.dx_disc_first_wgrad_size(R, T, p, cout, k, s, pad, nb.data_ptr())
        need = int(nb.item())
        N = conv_out(-(-T // p), k, s, pad)
        for cin, cout, k, s, g, pad in self.LAYERS[1:]:
            L.dx_disc_wgrad_size(R * p, N, cin, cout, g, k, s, pad, nb.data_ptr(), None)
            need = max(need, int(nb.item()))
            N = conv_out(N, k, s, pad)
        L.dx_disc_post_wgrad_size(R * p, N, POST[0], POST[2], nb.data_ptr())
        return max(need, int(nb.item()))

    def _run_wgrad(self, x2, score, fmaps, B, p, gw, dz, ws, zero):
        """The discriminator step of one sub-discriminator (csrc/dx_disc_wgrad.hip): x2 (2B, T) its input, score (2B, N, p) and the
        channels-last maps of a pass, real rows first; gw -> ONE device float, the upstream gradient of its discriminator loss; dz two
        buffers for the pre-activation gradients of all 2B rows; ws the workspace; zero -> a device zero (dx_disc_conv_dgrad's
        feature-matching weight) -> {layer: (dW (Cout, Cin / groups, taps), db)} of the folded pairs.  Top down, each layer's weight
        gradient launched before its data gradient, so the two dz buffers suffice."""
        L, st, dev = lib(), _stream(score.device), score.device
        P, D = self._device_weights(), self._dgrad_weights()
        N, C, R = score.shape[1], POST[0], 2 * B
        last = fmaps[-1]
        cur, nxt = dz
        out = {}
        dW, db = _fresh((POST[1], C, POST[2]), dev), _fresh((POST[1],), dev)
        L.dx_disc_post_wgrad(score.data_ptr(), N * p, 1, p, P['conv_post'][0].data_ptr(), last.data_ptr(), cur.data_ptr(), N * p * C, C, p * C, gw,
                             2.0 / (score.numel() // 2), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), R * p, B * p, p, N, C, POST[2], st)
        out['conv_post'] = (dW, db)
        for i in range(len(self.LAYERS) - 1, 0, -1):
            cin, cout, k, s, grp, pad = self.LAYERS[i]
            below = fmaps[i - 1]
            n_in, n_out = below.shape[1], fmaps[i].shape[1]
            dW, db = _fresh((cout, cin // grp, k), dev), _fresh((cout,), dev)
            L.dx_disc_wgrad(below.data_ptr(), n_in * p * cin, cin, p * cin, cur.data_ptr(), n_out * p * cout, cout, p * cout, dW.data_ptr(),
                            db.data_ptr(), ws.data_ptr(), ws.numel(), R * p, p, n_in, cin, cout, grp, k, s, pad, st)
            out[f'convs.{i}'] = (dW, db)
            L.dx_disc_conv_dgrad(cur.data_ptr(), n_out * p * cout, cout, p * cout, D[i].data_ptr(), nxt.data_ptr(), below.data_ptr(),
                                 below.data_ptr(), n_in * p * cin, cin, p * cin, zero, 0.0, R * p, p, n_in, cin, cout, grp, k, s, pad, 1, 0, st)
            cur, nxt = nxt, cur
        _, cout, k, s, _, pad = self.LAYERS[0]
        dW, db = _fresh((cout, 1, k), dev), _fresh((cout,), dev)
        L.dx_disc_first_wgrad(x2.data_ptr(), x2.shape[1], x2.shape[1], cur.data_ptr(), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), R, p,
                              cout, k, s, pad, st)
        out['convs.0'] = (dW, db)
        return out

    def _run(self, x2, p, alloc):
        """x2 (R, T) fp32 contiguous on the device, period p (1: no folding) -> (scores (R, N, p), [channels-last feature maps
        (R, N_i, p, C_i)]): one launch per layer."""
        L, st, bf16 = lib(), _stream(x2.device), PRECISIONS[self.precision]
        P = self._device_weights()
        R, T = x2.shape
        dev = x2.device
        cin, cout, k, s, _, pad = self.LAYERS[0]
        N = conv_out(-(-T // p), k, s, pad)
        w, b = P['convs.0']
        cur = alloc((R, N, p, cout), dev)
        L.dx_disc_first(x2.data_ptr(), T, T, w.data_ptr(), b.data_ptr(), cur.data_ptr(), R, p, cout, k, s, pad, st)
        fmaps = [cur]
        for i, (cin, cout, k, s, g, pad) in enumerate(self.LAYERS[1:], 1):
            w, b = P[f'convs.{i}']
            nout = conv_out(N, k, s, pad)
            out = alloc((R, nout, p, cout), dev)
            L.dx_disc_conv(cur.data_ptr(), N * p * cin, cin, p * cin, w.data_ptr(), b.data_ptr(), out.data_ptr(), nout * p * cout, cout,
                           p * cout, R * p, p, N, cin, cout, g, k, s, pad, 1, bf16, st)
            fmaps.append(out)
            cur, N = out, nout
        w, b = P['conv_post']
        score = alloc((R, N, p), dev)
        C = POST[0]
        L.dx_disc_post(cur.data_ptr(), N * p * C, C, p * C, w.data_ptr(), b.data_ptr(), score.data_ptr(), N * p, 1, p, R * p, p, N, C, POST[2], st)
        return score, fmaps


def _views_p(score, fmaps):
    """channels-last buffers -> the reference's (x (R, N p), [fmap (R, C, H, p)])."""
    R = score.shape[0]
    return score.view(R, -1), [f.permute(0, 3, 1, 2) for f in fmaps] + [score.unsqueeze(1)]


def _views_s(score, fmaps):
    """channels-last buffers -> the reference's (x (R, N), [fmap (R, C, N)])."""
    R = score.shape[0]
    return score.view(R, -1), [f.squeeze(2).permute(0, 2, 1) for f in fmaps] + [score.view(R, 1, -1)]


class DiscriminatorP(_SubDiscriminator):
    """One period sub-discriminator (discriminators.py:28-66): (5, 1) convolutions over the period-folded signal."""
    LAYERS = MPD_LAYERS

    def __init__(self, period, precision='f32'):
        super().__init__()
        self.period = int(period)
        self._init_layers(_WNConv, True, precision)

    def forward(self, x):
        """x (B, 1, T) -> (scores (B, n), [6 feature maps (B, C, H, p)])."""
        _check_inputs(x)
        _check_reflect(x.shape[2], (self.period,))
        _check_run(self, x)
        return _views_p(*self._run(x.reshape(x.shape[0], -1).contiguous(), self.period, _fresh))


class DiscriminatorS(_SubDiscriminator):
    """One scale sub-discriminator (discriminators.py:98-124): grouped k = 41 Conv1d layers."""
    LAYERS = MSD_LAYERS

    def __init__(self, use_spectral_norm=False, precision='f32'):
        super().__init__()
        self.use_spectral_norm = bool(use_spectral_norm)
        self._init_layers(_SNConv if use_spectral_norm else _WNConv, False, precision)

    def forward(self, x):
        """x (B, 1, T) -> (scores (B, n), [8 feature maps (B, C, N)])."""
        _check_inputs(x)
        _check_run(self, x)
        return _views_s(*self._run(x.reshape(x.shape[0], -1).contiguous(), 1, _fresh))


class _MultiDiscriminator(nn.Module):
    def refresh_weights(self, folded=None):
        """``folded``: {'discriminators.<i>.<layer>': (W, bias)}, see _SubDiscriminator.refresh_weights; a sub-discriminator none of whose
        layers is named (the spectral-normed one) folds its own parameters as before."""
        for i, d in enumerate(self.discriminators):
            prefix = f'discriminators.{i}.'
            own = None if folded is None else {k[len(prefix):]: v for k, v in folded.items() if k.startswith(prefix)}
            d.refresh_weights(own or None)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.refresh_weights()
        return out

    def forward(self, y, y_hat):
        """y, y_hat (B, 1, T) fp32 on the device -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) as the reference returns them."""
        _check_inputs(y, y_hat)
        self._check_shape(y.shape[2])
        _check_run(self, y, y_hat)
        B = y.shape[0]
        x2 = torch.cat([y.detach().reshape(B, -1), y_hat.detach().reshape(B, -1)], 0)
        y_d_rs, y_d_gs, fmap_rs, fmap_gs = [], [], [], []
        for score, fmaps in (self._views(*raw) for raw in self._run(x2, _fresh)):
            y_d_rs.append(score[:B])
            y_d_gs.append(score[B:])
            fmap_rs.append([f[:B] for f in fmaps])
            fmap_gs.append([f[B:] for f in fmaps])
        return y_d_rs, y_d_gs, fmap_rs, fmap_gs

    def _check_shape(self, T):
        pass


class MultiPeriodDiscriminator(_MultiDiscriminator):
    """Five period sub-discriminators, periods 2, 3, 5, 7, 11 (discriminators.py:69-91): 30 launches for both inputs."""

    def __init__(self, precision='f32'):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorP(p, precision) for p in PERIODS])

    def _check_shape(self, T):
        _check_reflect(T, PERIODS)

    _views = staticmethod(_views_p)

    def _run(self, x2, alloc):
        """-> per sub-discriminator (scores, feature maps) as the kernels' channels-last buffers."""
        return [d._run(x2, d.period, alloc) for d in self.discriminators]


class MultiScaleDiscriminator(_MultiDiscriminator):
    """Three scale sub-discriminators, the first spectral-normed, the others fed through AvgPool1d(4, 2, padding=2)
    (discriminators.py:127-156): 26 launches for both inputs."""

    def __init__(self, precision='f32'):
        super().__init__()
        self.discriminators = nn.ModuleList([DiscriminatorS(True, precision), DiscriminatorS(False, precision),
                                             DiscriminatorS(False, precision)])
        self.meanpools = nn.ModuleList([nn.Module(), nn.Module()])      # the reference's two AvgPool1d: no parameters

    _views = staticmethod(_views_s)

    def _run(self, x2, alloc, inputs=None):
        """``inputs``: a list that receives the (R, T_i) input of each sub-discriminator (the waveforms, then the two pooled buffers)."""
        out = []
        for i, d in enumerate(self.discriminators):
            if i:
                R, T = x2.shape
                pooled = alloc((R, T // 2 + 1), x2.device)
                lib().dx_disc_pool(x2.data_ptr(), pooled.data_ptr(), R, T, _stream(x2.device))
                x2 = pooled
            if inputs is not None:
                inputs.append(x2)
            out.append(d._run(x2, 1, alloc))
        return out


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


def _loss_rows(pairs, kind, set_id, keep):
    rows = []
    for r, g in pairs:
        r, g = _dense_pair(r, g)
        if r.numel() == 0:
            raise ValueError('a loss over an empty tensor')
        keep += [r, g]
        rows.append([r.data_ptr(), g.data_ptr(), r.numel(), kind + 2 * set_id])
    return rows


class _LossPlan:
    """The device table of dx_disc_losses for a fixed list of tensors, and its workspace."""

    def __init__(self, rows, n_sets, device):
        if device.type != 'cuda':
            raise RuntimeError('the GAN losses run on the GPU (csrc/dx_disc.hip); there is no CPU path')
        self.n, self.n_sets = len(rows), n_sets
        self.max_count, self.total = max(r[2] for r in rows), sum(r[2] for r in rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(device)
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
    keep = []
    out = _LossPlan(_loss_rows(pairs, 0, 0, keep), 1, pairs[0][0].device).run()
    return out[0], [out[3 + 3 * i] for i in range(len(pairs))], [out[3 + 3 * i + 1] for i in range(len(pairs))]


def generator_loss(disc_outputs):
    """-> (loss, gen_losses) as discriminators.py:177-185."""
    outs = list(disc_outputs)
    _check_loss_inputs(outs)
    keep = []
    out = _LossPlan(_loss_rows([(t, t) for t in outs], 0, 0, keep), 1, outs[0].device).run()
    return out[1], [out[3 + 3 * i + 2] for i in range(len(outs))]


def feature_loss(fmap_r, fmap_g):
    """-> 2 x the sum over all feature maps of mean |r - g| (discriminators.py:188-194)."""
    pairs = [(rl, gl) for dr, dg in zip(fmap_r, fmap_g) for rl, gl in zip(dr, dg)]
    _check_loss_inputs([t for p in pairs for t in p])
    keep = []
    return _LossPlan(_loss_rows(pairs, 1, 0, keep), 1, pairs[0][0].device).run()[2]


def _checkpoint(checkpoint) -> dict:
    if isinstance(checkpoint, (str, os.PathLike)):
        checkpoint = torch.load(checkpoint, map_location='cpu')
    if not isinstance(checkpoint, dict) or 'mpd' not in checkpoint or 'msd' not in checkpoint:
        raise TypeError("a discriminator checkpoint is a dict with 'mpd' and 'msd' state dicts (the reference's do_* files)")
    return checkpoint


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
        self.mpd = MultiPeriodDiscriminator(precision)
        self.msd = MultiScaleDiscriminator(precision)
        self.mpd.load_state_dict(state['mpd'], strict=True)
        self.msd.load_state_dict(state['msd'], strict=True)
        self.mpd.to(self.device).eval()
        self.msd.to(self.device).eval()
        self._plans = {}

    def _pass(self, y, y_hat, differentiable=False, train=False):
        _check_inputs(y, y_hat)
        _check_reflect(y.shape[2], PERIODS)
        if train:
            _check_train(self, y)
        elif differentiable:
            _check_differentiable(self, y, y_hat)
        else:
            _check_run(self.mpd, y, y_hat)
        B, _, T = y.shape
        key = (B, T, y.device)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = {'f': _Arena(), 's': _Arena(), 'loss': None, 'pass': 0, 'bwd': None, 'gw': {}}
        plan['pass'] += 1
        x2 = torch.cat([y.detach().reshape(B, -1), y_hat.detach().reshape(B, -1)], 0)
        plan['f'].reset()
        plan['s'].reset()
        mpd = self.mpd._run(x2, plan['f'])
        plan['inputs'] = [x2] * len(PERIODS)         # the (2B, T_i) input of every sub-discriminator, for the first layers' weight gradients
        msd = self.msd._run(x2, plan['s'], plan['inputs'])
        return plan, B, mpd, msd

    def losses(self, y, y_hat) -> dict:
        plan, B, mpd, msd = self._pass(y, y_hat)
        return self._losses(plan, B, mpd, msd, y.device)

    def _losses(self, plan, B, mpd, msd, device):
        if plan['loss'] is None:
            rows, keep = [], []
            for s, outs in enumerate((mpd, msd)):
                rows += _loss_rows([(sc[:B], sc[B:]) for sc, _ in outs], 0, s, keep)
                rows += _loss_rows([(f[:B], f[B:]) for sc, fm in outs for f in fm + [sc]], 1, s, keep)
            plan['loss'] = _LossPlan(rows, 2, device)
        out = plan['loss'].run()
        return {name: out[i] for i, name in enumerate(LOSS_NAMES)}

    # ---- backward to the generated waveform (csrc/dx_disc_bwd.hip) -------------------------------------------------------------------
    def _forward_kept(self, y, y_hat):
        """One pass whose feature maps stay in the plan for a backward -> (state, the four generator-side losses)."""
        plan, B, mpd, msd = self._pass(y, y_hat, differentiable=True)
        six = self._losses(plan, B, mpd, msd, y.device)
        state = (plan, plan['pass'], B, y.shape[2], mpd, msd)
        return state, {name: six[name] for name in GEN_LOSS_NAMES}

    def _backward(self, state, gw):
        """gw: fp32 device tensor of 4, the upstream gradients in GEN_LOSS_NAMES order -> dy_hat (B, 1, T)."""
        plan, stamp, B, T, mpd, msd = state
        if plan['pass'] != stamp:
            raise RuntimeError('the discriminators\' feature maps of this pass were overwritten by a later pass at the same (B, T): '
                               'call backward() before the next losses() / generator_losses() / generator_loss_grad() at that shape')
        dev = gw.device
        if plan['bwd'] is None:
            biggest = max(f.numel() // 2 for _, fm in mpd + msd for f in fm)
            plan['bwd'] = {'dz': (_fresh((biggest,), dev), _fresh((biggest,), dev)),
                           'pooled': [_fresh((B, msd[i][1][0].shape[1]), dev) for i in (1, 2)]}
        dz, pooled = plan['bwd']['dz'], plan['bwd']['pooled']
        dy = _fresh((B, T), dev)
        for i, (d, (score, fmaps)) in enumerate(zip(self.mpd.discriminators, mpd)):
            d._run_bwd(score, fmaps, B, T, d.period, gw, 0, 1, dz, dy, i > 0)
        subs = self.msd.discriminators
        subs[0]._run_bwd(*msd[0], B, T, 1, gw, 2, 3, dz, dy, True)
        T1, T2 = pooled[0].shape[1], pooled[1].shape[1]
        subs[1]._run_bwd(*msd[1], B, T1, 1, gw, 2, 3, dz, pooled[0], False)
        subs[2]._run_bwd(*msd[2], B, T2, 1, gw, 2, 3, dz, pooled[1], False)
        L, st = lib(), _stream(dev)
        L.dx_disc_pool_bwd(pooled[1].data_ptr(), pooled[0].data_ptr(), B, T1, 1, st)
        L.dx_disc_pool_bwd(pooled[0].data_ptr(), dy.data_ptr(), B, T, 1, st)
        return dy.view(B, 1, T)

    def generator_losses(self, y, y_hat) -> dict:
        """-> {loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s}: the bits of ``losses()``, differentiable with respect to ``y_hat`` (only).
        The backward must run before the next pass at the same (B, T): the feature maps live in the per-shape plan."""
        out = _GeneratorLosses.apply(y_hat, self, y)
        return dict(zip(GEN_LOSS_NAMES, out))

    def generator_loss_grad(self, y, y_hat, weights=(1.0, 1.0, 1.0, 1.0)):
        """-> ({the four generator-side losses}, d sum_i weights[i] loss_i / d y_hat (B, 1, T)), without autograd.  ``weights``: four
        floats or an fp32 device tensor of 4, in the order loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s."""
        with torch.no_grad():
            state, four = self._forward_kept(y, y_hat)
            plan = state[0]
            if torch.is_tensor(weights):
                if weights.shape != (4,) or weights.dtype != torch.float32 or weights.device != y.device:
                    raise ValueError('weights: four floats or an fp32 tensor of 4 on the inputs\' device')
                gw = weights.detach().contiguous()
            else:
                key = tuple(float(w) for w in weights)
                if len(key) != 4:
                    raise ValueError('weights: four floats or an fp32 tensor of 4 on the inputs\' device')
                gw = plan['gw'].get(key)
                if gw is None:                       # uploaded once per plan: a captured graph must not copy from host memory
                    gw = plan['gw'][key] = torch.tensor(key, dtype=torch.float32).to(y.device)
            return four, self._backward(state, gw)

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
            _check_inputs(y, y_hat)
            _check_reflect(y.shape[2], PERIODS)
            _check_train(self, y)
            dev, key = y.device, None
            if torch.is_tensor(weights):
                if weights.shape != (2,) or weights.dtype != torch.float32 or weights.device != dev:
                    raise ValueError('weights: two floats or an fp32 tensor of 2 on the inputs\' device')
                gw = weights.detach().contiguous()
            else:
                key = tuple(float(w) for w in weights)
                if len(key) != 2:
                    raise ValueError('weights: two floats or an fp32 tensor of 2 on the inputs\' device')
            if n:
                for c in self._spectral_layers():
                    power_iterate(c.weight_orig, c.weight_u, c.weight_v, n)
                for d in self.msd.discriminators:
                    if d.use_spectral_norm:
                        d.refresh_weights()
            plan, B, mpd, msd = self._pass(y, y_hat, train=True)
            six = self._losses(plan, B, mpd, msd, y.device)
            if key is not None:
                gw = plan['gw'].get(key)
                if gw is None:                       # uploaded once per plan, as generator_loss_grad's
                    gw = plan['gw'][key] = torch.tensor(key, dtype=torch.float32).to(dev)
            subs = list(zip(self.mpd.discriminators, mpd, [d.period for d in self.mpd.discriminators], [0] * len(mpd))) + \
                list(zip(self.msd.discriminators, msd, [1] * len(msd), [1] * len(msd)))
            inputs = plan['inputs']
            if plan.get('train') is None:
                biggest = max(f.numel() for _, fm in mpd + msd for f in fm)
                need = max(d._wgrad_workspace(2 * B, x.shape[1], p) for (d, _, p, _), x in zip(subs, inputs))
                plan['train'] = {'dz': (_fresh((biggest,), dev), _fresh((biggest,), dev)), 'zero': torch.zeros(1, dtype=torch.float32, device=dev),
                                 'ws': torch.empty(need, dtype=torch.uint8, device=dev)}
            tr = plan['train']
            grads = {'mpd': {}, 'msd': {}}
            for j, ((d, (score, fmaps), p, which), x) in enumerate(zip(subs, inputs)):
                pairs = d._run_wgrad(x, score, fmaps, B, p, gw.data_ptr() + 4 * which, tr['dz'], tr['ws'], tr['zero'].data_ptr())
                i = j if which == 0 else j - len(mpd)
                for name, (dw, db) in pairs.items():
                    conv = d.conv_post if name == 'conv_post' else d.convs[int(name[len('convs.'):])]
                    if folded and not isinstance(conv, _SNConv):
                        grads['msd' if which else 'mpd'][f'discriminators.{i}.{name}'] = (dw, db)
                    else:
                        _norm_backward(conv, f'discriminators.{i}.{name}', dw, db, grads['msd' if which else 'mpd'])
            return {'loss_disc_f': six['loss_disc_f'], 'loss_disc_s': six['loss_disc_s']}, grads

    def discriminator_backward(self, y, y_hat, weights=(1.0, 1.0), power_iterations=1):
        """``discriminator_loss_grad`` whose gradients are ADDED into each parameter's ``.grad`` (created where it is None) -> the two
        losses.  The parameters stay frozen leaves: an optimiser steps whatever has a ``.grad``, so the discriminator step is
        ``optim_d.zero_grad(); D.discriminator_backward(y, y_hat); optim_d.step(); D.mpd.refresh_weights(); D.msd.refresh_weights()``."""
        two, grads = self.discriminator_loss_grad(y, y_hat, weights, power_iterations)
        with torch.no_grad():
            for tag, module in (('mpd', self.mpd), ('msd', self.msd)):
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
        state, four = owner._forward_kept(y, y_hat)
        ctx.owner, ctx.state = owner, state
        return tuple(four[name].clone() for name in GEN_LOSS_NAMES)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        ref = next(g for g in grads if g is not None)
        gw = torch.stack([torch.zeros_like(ref) if g is None else g for g in grads]).float().reshape(4).contiguous()
        return ctx.owner._backward(ctx.state, gw), None, None


__all__ = ['DiscriminatorP', 'DiscriminatorS', 'MultiPeriodDiscriminator', 'MultiScaleDiscriminator', 'HiFiGanDiscriminators',
           'discriminator_loss', 'generator_loss', 'feature_loss']
