"""Training the HiFi-GAN generator on gfx950: ``HiFiGANGenerator.forward`` and the backward to every weight_g, weight_v and bias
(reference vocoder/finetune_hifigan.py:209-243, the generator step), f32 operands.

The forward with gradients runs ``generator_launches(config, 'f32', training=True)``: dx_voc_conv and dx_voc_post launches only, every
tensor in a buffer of its own.  ``backward_launches`` derives the backward from that list, in reverse:

  * every DATA gradient is a ``dx_voc_conv`` launch on a pack built here -- ``dgrad_weight``: a dilated 'same' conv's gradient is the conv
    of dY with the flipped, transposed weight; ``ups_dgrad_weight``: the gradient of ConvTranspose1d(k = 2u, stride u, padding u / 2) is a
    three-tap conv of the view (N u, Cout) -> (N, u Cout) of dY, a reshape that is free in the channels-last layout;
  * ``dx_voc_wgrad`` gives each layer's weight and bias gradient, ``dx_voc_act_bwd`` the leaky-ReLU, residual and mean-of-three steps
    between them, ``dx_voc_post_bwd`` all of conv_post (csrc/dx_vocoder_bwd.hip).

Weight norm is autograd's: the module folds ``torch._weight_norm(v, g, 0)`` on the device and pads V2's 8-channel stage with
``pad_folded_weights``; the autograd function takes the folded (weight, bias) pairs and returns their gradients, from which PyTorch
derives those of g and v (the padded channels' gradients fall away in ``cat``'s backward).

``generator_forward_folded`` is the same forward from folded leaves the caller owns (the fine-tuning loop).

Not here: the fused pair / chain in training, graph capture of the step, the discriminators' weight
gradients, the gradient to the mel, bf16 operands."""
from __future__ import annotations

import functools
import json

import torch

from ._lib import lib, packed as _packed, stream as _stream
from .vocoder import HOP, HiFiGanVocoder, _issue, check_config, generator_launches, pad_folded_weights


# ---- host-built operands of the data gradients --------------------------------------------------------------------------------------
def dgrad_weight(w):
    """W (Cout, Cin, k) of a dilated 'same' Conv1d -> the (Cin, Cout, k) weight whose conv of dY, same padding and dilation, is dX."""
    return w.flip(2).transpose(0, 1).contiguous()


def ups_dgrad_weight(w, u):
    """W (Cin, Cout, 2u) of ConvTranspose1d(stride u, padding u / 2) -> Wv (Cin, u Cout, 3): dX = conv1d(dYv, Wv, padding=1) on the view
    dYv (N, u Cout) of dY (N u, Cout).  Wv[:, r Cout + co, d + 1] = W[:, co, d u + r + u / 2] where that index is in [0, 2u), else 0."""
    cin, cout, k = w.shape
    if k != 2 * u or u % 2:
        raise ValueError(f'ups_dgrad_weight: a (Cin, Cout, 2u) weight with u even, got {tuple(w.shape)} for u = {u}')
    wv = w.new_zeros(cin, u, cout, 3)
    for d in (-1, 0, 1):
        for r in range(u):
            j = d * u + r + u // 2
            if 0 <= j < k:
                wv[:, r, :, d + 1] = w[:, :, j]
    return wv.reshape(cin, u * cout, 3)


# ---- the backward as a list (host only) ---------------------------------------------------------------------------------------------
class BackwardLaunches:
    """What ``backward_launches`` returns.  ``steps``: in order, dicts with 'kernel' ('post_bwd', 'conv', 'act_bwd', 'wgrad'), 'layer',
    'saved' (the forward tensors the step reads), 'reads' / 'writes' (gradient buffers) and the kernel's own shape fields; ``buffers``:
    {gradient buffer: {'scale' rows per mel frame, 'channels'}}; 'dy' is the upstream gradient (B, 256 T)."""

    def __init__(self, steps, buffers):
        self.steps, self.buffers = steps, buffers

    def __len__(self):
        return len(self.steps)


def backward_launches(config=None) -> BackwardLaunches:
    """The backward of ``generator_launches(config, 'f32', training=True)``, launch by launch in reverse.  For a residual step
    y = r + conv(lrelu x) with g = dy:  U = convT(g) (dx_voc_conv on the flipped pack, no bias, no lrelu), dW = wgrad(lrelu x, g),
    db = column sums of g, and d x = lrelu'(x) U, to which g is added where x is r (ResBlock2) or, for a ResBlock1 pair, when the
    first conv's input is reached.  A stage's mean of three: every ResBlock's incoming gradient is g3 = dsum / 3, one act_bwd."""
    return _backward_launches(json.dumps(check_config(config), sort_keys=True))


@functools.lru_cache(maxsize=None)
def _backward_launches(config_json):
    fwd = generator_launches(json.loads(config_json), 'f32', training=True)
    T = fwd.tensors
    steps, G = [], {}
    pending = {}                 # ResBlock1: {the pair's input tensor: the gradient of the pair's output}, until convs1 is reached

    def grad(name, like):        # the gradient buffer `name`, shaped as forward tensor `like`
        G.setdefault(name, dict(scale=T[like]['scale'], channels=T[like]['channels']))
        return name

    def step(kernel, layer, saved, reads, writes, **fields):
        steps.append(dict(kernel=kernel, layer=layer, saved=[s for s in saved if s], reads=[r for r in reads if r], writes=writes, **fields))

    def act_bwd(layer, x, u, r, like, gscale=1.0):
        """g.<like> (+)= gscale lrelu'(x) u + r: the first contribution writes, the later ones add."""
        out, acc = 'g.' + like, int('g.' + like in G)
        grad(out, like)
        step('act_bwd', layer, [x], [u, r, out if acc else None], [out], x=x, u=u, r=r, out=out, acc=acc, gscale=gscale,
             scale=T[like]['scale'], channels=T[like]['channels'])
        return out

    for ln in reversed(fwd.launches):
        layer, x, y, r = ln['layer'], ln['x'], ln['y'], ln['r']
        if ln['kind'] == 'post':
            step('post_bwd', layer, [x, 'audio'], ['dy'], [grad('g.' + x, x)], x=x, out='g.' + x, scale=ln['scale'], channels=ln['cin'])
            continue
        assert ln['kind'] == 'conv'
        gy = 'g.' + y
        if y.startswith('sum.') and r is not None:                       # a ResBlock's last conv adds into the stage's sum
            gy = 'g3.' + y
            if gy not in G:
                grad(gy, y)
                step('act_bwd', y, [], ['g.' + y], [gy], x=None, u='g.' + y, r=None, out=gy, acc=0, gscale=1.0 / 3.0,
                     scale=T[y]['scale'], channels=T[y]['channels'])
        up = ln['up']
        step('wgrad', layer, [x], [gy], [], x=x, gy=gy, cin=ln['cin'], cout=ln['cout'], taps=3 if up > 1 else ln['taps'], dil=ln['dil'],
             up=up, act=ln['lrelu'], scale=ln['scale'])
        if x == 'mel':                                                   # conv_pre: no gradient to the mel
            continue
        u = grad(f"U.{T[x]['scale']}x{T[x]['channels']}", x)                 # scratch of x's shape: read by the act_bwd that follows
        if up > 1:           # the three-tap conv of the view (N, up Cout) of g
            step('conv', layer, [], [gy], [u], gy=gy, out=u, pack='ups_dgrad', cin=up * ln['cout'], cout=ln['cin'], taps=3, dil=1, scale=ln['scale'])
        else:
            step('conv', layer, [], [gy], [u], gy=gy, out=u, pack='dgrad', cin=ln['cout'], cout=ln['cin'], taps=ln['taps'], dil=ln['dil'],
                 scale=ln['scale'])
        if r is not None and r != x:                                     # ResBlock1's second conv: x is mid; g waits for the pair's input
            pending[r] = gy
            act_bwd(layer, x, u, None, x)
        elif r is not None:                                              # ResBlock2: d x = g + lrelu'(x) U
            act_bwd(layer, x, u, gy, x)
        else:                                                            # ResBlock1's first conv, or a transposed conv
            act_bwd(layer, x, u, pending.pop(x, None), x)
    assert not pending
    return BackwardLaunches(steps, G)


# ---- the autograd function ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wgrad_bytes(B, N, cin, cout, taps, up):
    n = torch.zeros(1, dtype=torch.long)
    lib().dx_voc_wgrad_size(B, N, cin, cout, taps, up, n.data_ptr())
    return int(n.item())


@functools.lru_cache(maxsize=None)
def _post_bwd_bytes(B, N, C):
    n = torch.zeros(1, dtype=torch.long)
    lib().dx_voc_post_bwd_size(B, N, C, n.data_ptr())
    return int(n.item())


class _GeneratorFunction(torch.autograd.Function):
    """(mel, frames, config, layer names, w0, b0, w1, b1, ...) -> audio (B, 256 T); the weights are the folded, padded pairs."""

    @staticmethod
    def forward(ctx, mel, frames, config_json, names, *wb):
        config = json.loads(config_json)
        topo = generator_launches(config, 'f32', training=True)
        L, dev, st = lib(), mel.device, _stream(mel.device)
        B, n_mel, T = mel.shape
        weights = {name: (wb[2 * i].contiguous(), wb[2 * i + 1].contiguous()) for i, name in enumerate(names)}
        ups = {f'ups.{i}': u for i, u in enumerate(config['upsample_rates'])}
        packs = {}
        for name, (w, b) in weights.items():
            if name == 'conv_post':
                packs[name] = (w, b)
            elif name in ups:
                packs[name] = (_packed('voc', w, (w.shape[1], w.shape[0], 2, ups[name], 0), dev), b)
            else:
                packs[name] = (_packed('voc', w, (w.shape[0], w.shape[1], w.shape[2], 1, 0), dev), b)
        bufs = {name: torch.empty(B, T * t['scale'], t['channels'], dtype=torch.float32, device=dev) for name, t in topo.tensors.items()}
        audio = torch.empty(B, T * HOP, dtype=torch.float32, device=dev)
        at = {'mel': (mel.data_ptr(), n_mel * T, 1, T, 0), 'audio': (audio.data_ptr(), T * HOP, 0, 0, 0), None: None}
        at.update((name, (t.data_ptr(), t.shape[1] * t.shape[2], t.shape[2], 1, 0)) for name, t in bufs.items())
        for ln in topo.launches:
            _issue(L, ln, packs, at[ln['x']], at[ln['y']], at[ln['r']], frames.data_ptr(), B, T * ln['scale'], 0, None, st)
        ctx.config, ctx.names, ctx.ups, ctx.bufs, ctx.used = config, names, ups, bufs, False
        ctx.save_for_backward(mel, frames, audio, *wb)
        return audio

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        if ctx.used:
            raise RuntimeError('HiFiGANGenerator: a second backward through the same forward: the activations it kept are released by '
                               'the first one; run the forward again')
        mel, frames, audio, *wb = ctx.saved_tensors
        ctx.used = True
        saved, ctx.bufs = dict(ctx.bufs, mel=mel, audio=audio), None
        L, dev, st = lib(), mel.device, _stream(mel.device)
        B, n_mel, T = mel.shape
        weights = {name: (wb[2 * i].contiguous(), wb[2 * i + 1].contiguous()) for i, name in enumerate(ctx.names)}
        plan = backward_launches(ctx.config)
        last = {}                                                        # the step after which a buffer is dead
        for i, s in enumerate(plan.steps):
            for name in s['saved'] + s['reads'] + s['writes']:
                last[name] = i
        grads = {'dy': dy.reshape(B, T * HOP).float().contiguous()}
        out = {}
        fr = frames.data_ptr()

        def gbuf(name):
            if name not in grads:
                t = plan.buffers[name]
                grads[name] = torch.empty(B, T * t['scale'], t['channels'], dtype=torch.float32, device=dev)
            return grads[name]

        for i, s in enumerate(plan.steps):
            kernel, layer, N = s['kernel'], s['layer'], T * s['scale']
            if kernel == 'post_bwd':
                w, b = weights[layer]
                C = s['channels']
                dw, db = torch.empty_like(w), torch.empty_like(b)
                nbytes = _post_bwd_bytes(B, N, C)
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                L.dx_voc_post_bwd(saved[s['x']].data_ptr(), N * C, w.data_ptr(), audio.data_ptr(), grads['dy'].data_ptr(), T * HOP,
                                  gbuf(s['out']).data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes, fr, s['scale'], B, N, C, st)
                out[layer] = (dw, db)
            elif kernel == 'wgrad':
                w, b = weights[layer]
                dw, db = torch.empty_like(w), torch.empty_like(b)
                cin, cout, up = s['cin'], s['cout'], s['up']
                x = saved[s['x']]
                xs = (n_mel * T, 1, T) if s['x'] == 'mel' else (N * cin, cin, 1)
                nbytes = _wgrad_bytes(B, N, cin, cout, s['taps'], up)
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                L.dx_voc_wgrad(x.data_ptr(), *xs, grads[s['gy']].data_ptr(), N * up * cout, up * cout, 0, dw.data_ptr(), db.data_ptr(),
                               ws.data_ptr(), nbytes, fr, s['scale'], B, N, cin, cout, s['taps'], s['dil'], up, s['act'], st)
                out[layer] = (dw, db)
            elif kernel == 'conv':
                w, _ = weights[layer]
                cin, cout = s['cin'], s['cout']
                wd = ups_dgrad_weight(w, ctx.ups[layer]) if s['pack'] == 'ups_dgrad' else dgrad_weight(w)
                pack = _packed('voc', wd, (cout, cin, s['taps'], 1, 0), dev)
                L.dx_voc_conv(grads[s['gy']].data_ptr(), N * cin, cin, 1, pack.data_ptr(), None, gbuf(s['out']).data_ptr(), N * cout, None,
                              fr, s['scale'], B, N, cin, cout, s['taps'], s['dil'], 1, 0, 0, 0, st)
            else:
                x = saved[s['x']].data_ptr() if s['x'] else None
                r = grads[s['r']].data_ptr() if s['r'] else None
                u = grads[s['u']].data_ptr()
                L.dx_voc_act_bwd(x, u, r, gbuf(s['out']).data_ptr(), fr, s['scale'], B, N, s['channels'], s['gscale'], s['acc'], st)
            for name in s['saved'] + s['reads']:                         # the caching allocator orders the reuse on this stream
                if last[name] == i:
                    saved.pop(name, None)
                    grads.pop(name, None)
        flat = []
        for name in ctx.names:
            flat += list(out[name])
        return (None, None, None, None, *flat)


def generator_forward(module, x, lengths=None):
    """``HiFiGANGenerator.forward``."""
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != module.config['model_in_dim']:
        raise ValueError(f'HiFiGANGenerator: x must be a (B, {module.config["model_in_dim"]}, T) mel, got '
                         f'{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    params = list(module.parameters())
    dev = params[0].device
    if dev.type != 'cuda' or x.device.type != 'cuda':
        raise RuntimeError('HiFiGANGenerator runs on the GPU (gfx950 HIP kernels); there is no CPU path')
    training = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('HiFiGANGenerator: x requires grad, and there is no gradient to the mel (dx_voc_conv has no 80-column form)')
    B, _, T = x.shape
    if lengths is None:
        lengths = [T] * B
    if not training:
        key = tuple((p.data_ptr(), p._version) for p in params)
        if module._inference is None or module._inference[0] != key:
            state = {k: v.detach().cpu() for k, v in module.state_dict().items()}
            module._inference = (key, HiFiGanVocoder(state, config=module.config, device=dev, precision=module.precision))
        audio, _ = module._inference[1].infer_batch(x, lengths)
        return audio[:, None, :]
    weights = {}
    for name in module.layer_names():
        m = module.get_submodule(name)
        weights[name] = (torch._weight_norm(m.weight_v, m.weight_g, 0), m.bias)
    return _forward_folded(module, x, lengths, weights)


def generator_forward_folded(module, x, folded, lengths=None):
    """``HiFiGANGenerator.forward`` in training from caller-owned folded weights: ``folded`` {layer: (W, bias)}, W in weight_v's shape --
    leaves that require grad, e.g. vocoder_optim.NormedAdamW(..., leaves=True).folded().  After ``backward()`` their ``.grad`` is the
    gradient of the folded weight; torch's weight-norm fold and its backward never run.  The caller vouches that W is the fold of the
    module's parameters."""
    if not torch.is_tensor(x) or x.dim() != 3 or x.shape[1] != module.config['model_in_dim']:
        raise ValueError(f'HiFiGANGenerator: x must be a (B, {module.config["model_in_dim"]}, T) mel, got '
                         f'{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    names = module.layer_names()
    if sorted(folded) != sorted(names):
        raise ValueError('generator_forward_folded: folded must hold exactly the generator\'s layers')
    for name in names:
        w, v = folded[name][0], module.get_submodule(name).weight_v
        if w.shape != v.shape or w.device != v.device or w.dtype != torch.float32:
            raise ValueError(f'generator_forward_folded: the folded weight of {name} must be fp32 of shape {tuple(v.shape)} on {v.device}')
    if x.device.type != 'cuda' or folded[names[0]][0].device.type != 'cuda':
        raise RuntimeError('HiFiGANGenerator runs on the GPU (gfx950 HIP kernels); there is no CPU path')
    if torch.is_grad_enabled() and x.requires_grad:
        raise RuntimeError('HiFiGANGenerator: x requires grad, and there is no gradient to the mel (dx_voc_conv has no 80-column form)')
    if lengths is None:
        lengths = [x.shape[2]] * x.shape[0]
    return _forward_folded(module, x, lengths, {name: folded[name] for name in names})


def _forward_folded(module, x, lengths, weights):
    """The training forward after the fold: weights {layer: (folded weight, bias)} in layer order, unpadded."""
    B, _, T = x.shape
    dev = weights['conv_pre'][0].device
    if module.precision != 'f32':
        raise RuntimeError(f"HiFiGANGenerator: gradients exist for precision 'f32' only, got {module.precision!r}")
    mel = x.detach().float().contiguous()
    if torch.is_tensor(lengths):
        frames = lengths.to(device=dev, dtype=torch.int32).clamp(0, T).contiguous()
    else:
        frames = torch.tensor([int(v) for v in lengths], dtype=torch.int32).clamp(0, T).to(dev)
    if frames.shape != (B,):
        raise ValueError(f'HiFiGANGenerator: {frames.numel()} lengths for a batch of {B}')
    names = tuple(module.layer_names())
    weights = pad_folded_weights(weights, module.config)
    flat = [t for name in names for t in weights[name]]
    audio = _GeneratorFunction.apply(mel, frames, json.dumps(module.config, sort_keys=True), names, *flat)
    return audio[:, None, :]
