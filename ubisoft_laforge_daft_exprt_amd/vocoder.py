"""HiFi-GAN vocoder (generators V1, V2 and V3) on gfx950: mel spectrogram -> waveform (reference src/daft_exprt/vocoder/hifigan.py).

``HiFiGANGenerator`` owns the reference generator's weight-normed state-dict layout (234 tensors for V1 and V2, 69 for V3); ``HiFiGanVocoder`` /
``load_hifigan_vocoder`` are drop-ins for the reference helpers (``.infer``: one utterance, numpy in or out) and add
``.infer_batch``: a padded (B, 80, T_max) mel batch on the device -- what ``DaftExprt.inference`` and ``GraphedSynthesizer`` return --
to (B, 256 T_max) audio on the device, row b bitwise equal to ``mel[b, :, :lengths[b]]`` vocoded alone -- and ``.stream``: the same
samples, bit for bit, in chunks of a few mel frames from ring buffers of fixed size (``stream_plan``, ``VocoderStream``).

Weight norm is folded once, at load time (``torch._weight_norm`` over dim 0, what ``remove_weight_norm`` computes: per OUTPUT channel
for the Conv1d layers, per INPUT channel for the ConvTranspose1d ones, whose weight is (Cin, Cout, k)).  Every convolution runs in
csrc/dx_vocoder.hip; there is no PyTorch fallback.  Checkpoints are read from a local path only: nothing here downloads.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import torch
from torch import nn

from ._lib import lib, packed as _packed, stream as _stream
from .graphs import capture

NEG_SLOPE = 0.1     # leaky-ReLU slope before every convolution (applied inside the kernels)
HOP = 256           # waveform samples per mel frame: the product of the four upsampling factors

# HiFi-GAN V1, the default configuration (V2 and V3: v2_config, v3_config below): 80 mel bins into 512 channels; four (factor, transposed-conv width)
# stages that halve the channels; three ResBlock1 per stage with kernel widths 3, 7, 11, each at dilations 1, 3, 5; 22.05 kHz.
N_MELS, WIDTH = 80, 512
STAGES = ((8, 16), (8, 16), (2, 4), (2, 4))
RESBLOCK_WIDTHS = (3, 7, 11)
RESBLOCK_DILATIONS = (1, 3, 5)


def v1_config() -> dict:
    """The V1 configuration in the key names of the reference's generator config dicts."""
    return dict(sampling_rate=22050, model_in_dim=N_MELS, upsample_initial_channel=WIDTH, resblock='1',
                upsample_rates=[f for f, _ in STAGES], upsample_kernel_sizes=[k for _, k in STAGES],
                resblock_kernel_sizes=list(RESBLOCK_WIDTHS), resblock_dilation_sizes=[list(RESBLOCK_DILATIONS) for _ in RESBLOCK_WIDTHS])


def v2_config() -> dict:
    """HiFi-GAN V2: V1 at a quarter of the width (128 channels into stages of 64, 32, 16 and 8)."""
    return dict(v1_config(), upsample_initial_channel=128)


def v3_config() -> dict:
    """HiFi-GAN V3: 256 channels, three stages (8, 8, 4) of 128, 64 and 32 channels, three ResBlock2 per stage (two dilated convs with
    a residual each) of widths 3, 5, 7."""
    return dict(sampling_rate=22050, model_in_dim=N_MELS, upsample_initial_channel=256, resblock='2', upsample_rates=[8, 8, 4],
                upsample_kernel_sizes=[16, 16, 8], resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]])


CONFIGS = {'v1': v1_config, 'v2': v2_config, 'v3': v3_config}     # the whitelist: the kernels are instantiated per width
DEFAULT_CONFIG = v1_config()
# operand mode of the conv kernels (the C ABI's `bf16` argument).  'bf16x3': split bf16 -- fp32 storage, every operand hi + lo in bf16,
# every product on three bf16 MFMAs (~16 mantissa bits); inference only, and the launch list is the f32 one (no chain launches).
PRECISIONS = {'f32': 0, 'bf16': 1, 'bf16x3': 2}
MIN_WIDTH = 16                               # one MFMA column block: a narrower stage (V2's last, 8 channels) runs zero-padded to it
WORKSPACE_BYTES_PER_FRAME = 5 * 8192 * 4    # V1: five fp32 activation buffers of at most 8192 values per mel frame (C x samples per frame)
DEFAULT_WORKSPACE_BYTES = 4 << 30            # infer_batch's default bound: larger batches run in chunks of utterances
# The ResBlock2 shapes (precision, channels, kernel width) that run as one dx_voc_chain launch: those for which it was measured faster
# than two dx_voc_conv launches (tools/bench_vocoder_chain.py).  With bf16 operands the block is bound by its
# traffic and the fused form, which never writes x1, wins at widths 3 and 5; at width 7 the 36-row halo makes it compute 2.5 times
# the first conv and it loses, as it does at every width in f32 mode, where the MFMAs run at the vector rate.  Every other shape, the
# 128-wide stage among them (the kernel has no instantiation for it), runs as two dx_voc_conv launches.
CHAIN_SHAPES = frozenset(('bf16', c, k) for c in (64, 32) for k in (3, 5))


def check_config(config) -> dict:
    """None -> V1; V1, V2 and V3 (lists or tuples alike) pass; any other configuration raises NotImplementedError: there is no
    fallback."""
    if config is None:
        return v1_config()

    def canon(v):
        return tuple(canon(x) for x in v) if isinstance(v, (list, tuple)) else str(v)
    got = {k: canon(v) for k, v in dict(config).items()}
    if not any(got == {k: canon(v) for k, v in make().items()} for make in CONFIGS.values()):
        raise NotImplementedError('the gfx950 HiFi-GAN kernels implement exactly three configurations, '
                                  + '; '.join(f'{name.upper()} ({make()})' for name, make in CONFIGS.items()) + f'; got {dict(config)}')
    return dict(config)


def stage_widths(config=None, padded=True) -> list:
    """Channels of each upsampling stage; ``padded``: as the kernels run them (at least MIN_WIDTH)."""
    cfg = check_config(config)
    widths = [int(cfg['upsample_initial_channel']) >> (i + 1) for i in range(len(cfg['upsample_rates']))]
    return [max(c, MIN_WIDTH) for c in widths] if padded else widths


def workspace_bytes_per_frame(config=None) -> int:
    """Bytes of ``infer_batch``'s activation workspace per mel frame of the longest row: five fp32 buffers of the widest tensor (padded
    channels x samples per frame).  V1: WORKSPACE_BYTES_PER_FRAME."""
    return 5 * 4 * max(t['channels'] * t['scale'] for t in generator_launches(config).tensors.values())


def pad_folded_weights(weights: dict, config=None) -> dict:
    """{layer: (folded weight, bias)} with every stage narrower than MIN_WIDTH (V2's last: 8 channels) zero-padded to it: the stage's
    transposed conv gets zero weights and a zero bias for output channels 8-15, its ResBlock convs zero rows, columns and biases there,
    and conv_post zero weights for input channels 8-15.  Those channels are then exactly 0 through every lrelu, residual and
    (y + v) / 3 -- a sum of zeros plus a zero bias -- and the real channels get the same sums plus added zeros, so the waveform is the
    unpadded generator's.  Layers of the other stages are returned as they are."""
    cfg = check_config(config)
    n_blocks = len(cfg['resblock_kernel_sizes'])
    out = dict(weights)

    def pad(name, dims):                 # zero-pad the listed dims of the weight (and the bias, if dim 0 of a Conv1d is among them)
        w, b = out[name]
        for d in dims:
            if w.shape[d] < MIN_WIDTH:
                shape = list(w.shape)
                shape[d] = MIN_WIDTH - w.shape[d]
                w = torch.cat([w, w.new_zeros(shape)], dim=d)
        if b.shape[0] < MIN_WIDTH and name != 'conv_post':
            b = torch.cat([b, b.new_zeros(MIN_WIDTH - b.shape[0])])
        out[name] = (w.contiguous(), b.contiguous())

    real = stage_widths(cfg, padded=False)
    for i, c in enumerate(real):
        if c >= MIN_WIDTH:
            continue
        pad(f'ups.{i}', (1,))                                         # ConvTranspose1d weight is (Cin, Cout, k)
        for name in weights:
            if name.startswith('resblocks.') and i * n_blocks <= int(name.split('.')[1]) < (i + 1) * n_blocks:
                pad(name, (0, 1))
        pad('conv_post', (1,))
    return out


# ---- the generator's launches (host only) ----------------------------------------------------------------------------------------
class GeneratorLaunches:
    """What ``generator_launches`` returns, shared between its callers (copy before writing).  ``tensors``: {name: {'scale' samples per
    mel frame, 'channels', 'slot'}} for every tensor between two layers; ``launches``, ``len()`` of them: in order, each a dict (kind
    'conv' / 'pair' / 'chain' / 'post', layer names, the names of its tensors 'x', 'y', 'r', the shape, 'scale' = tile rows per frame,
    and its 'left' / 'right' reach in rows of x)."""

    def __init__(self, tensors, launches):
        self.tensors, self.launches = tensors, launches

    def __len__(self):
        return len(self.launches)


def generator_launches(config=None, precision='f32', training=False) -> GeneratorLaunches:
    """The generator as the launches that compute it, built once per (configuration, precision): what ``infer_batch`` issues on whole
    tensors and ``stream_plan`` schedules on rings.  A ResBlock runs one of three ways: a ResBlock2 of a shape that is faster fused as
    one 'chain'; a ResBlock1 pair at 64 channels or fewer as one 'pair'; anything else as a 'conv' per convolution, a ResBlock1's
    through a 'mid' tensor.
    'slot': which fifth of ``infer_batch``'s workspace holds the tensor -- 0: conv_pre and the stage sums, 1: a stage's transposed conv,
    2 and 3: a ResBlock's x0 and x1, 4: mid.  Two tensors share a slot only when the first is dead before the second is written, and no
    launch reads and writes one slot (tests/test_vocoder_launches_cpu.py walks the launches to check both).
    ``training``: the list ``HiFiGANGenerator.forward`` runs when gradients are wanted ('f32' only): 'conv' and 'post' launches alone,
    and every tensor in a 'slot' of its own, so that the input of every convolution -- conv_pre, each ups.i, each ResBlock's x_p and
    mid_p, each sum.i -- is still there when ``vocoder_train.backward_launches`` reads it."""
    if precision not in PRECISIONS:
        raise ValueError(f'generator_launches: precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
    if training and precision != 'f32':
        raise ValueError(f"generator_launches: the training list exists for precision 'f32' only, got {precision!r}")
    return _generator_launches(json.dumps(check_config(config), sort_keys=True), precision, bool(training))       # lists and tuples dump alike


@functools.lru_cache(maxsize=None)
def _generator_launches(config_json, precision, training=False):
    cfg = json.loads(config_json)
    c = cfg['upsample_initial_channel']
    T, L = {}, []

    def tensor(name, scale, channels, slot):
        T[name] = dict(scale=scale, channels=channels, slot=len(T) if training else slot)
        return name

    def launch(layer, x, y, cin, cout, taps, dil, up, lrelu, acc, scale, reach, r=None, kind='conv', **second):
        L.append(dict(kind=kind, layer=layer, x=x, y=y, r=r, cin=cin, cout=cout, taps=taps, dil=dil, up=up, lrelu=lrelu, acc=acc,
                      scale=scale, left=reach, right=reach, **second))

    x, scale = tensor('conv_pre', 1, c, 0), 1
    launch('conv_pre', 'mel', x, cfg['model_in_dim'], c, 7, 1, 1, 0, 0, 1, 3)
    ks, ds = cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes']
    resblock2 = str(cfg['resblock']) == '2'
    for i, (u, cs) in enumerate(zip(cfg['upsample_rates'], stage_widths(cfg))):     # cs: the stage's channels as they run (padded)
        up_out = tensor(f'ups.{i}', scale * u, cs, 1)
        launch(f'ups.{i}', x, up_out, c, cs, 2, 1, u, 1, 0, scale, 1)
        scale, c = scale * u, cs
        total = tensor(f'sum.{i}', scale, c, 0)
        for j, k in enumerate(ks):
            name, src, h = f'resblocks.{i * len(ks) + j}', up_out, (k - 1) // 2
            last = len(ds[j]) - 1
            if not training and resblock2 and last == 1 and (precision, c, k) in CHAIN_SHAPES:    # both dilations of the ResBlock2 in one launch
                launch(f'{name}.convs.0', src, total, c, c, k, ds[j][0], 1, 1, min(j, 2), scale, (ds[j][0] + ds[j][1]) * h, kind='chain',
                     layer2=f'{name}.convs.1', dil2=ds[j][1])
                continue
            for p, d in enumerate(ds[j]):
                dst = total if p == last else tensor(f'{name}.x{p}', scale, c, 2 + p)
                acc = min(j, 2) if p == last else 0           # the stage sum: first ResBlock writes, second adds, third adds and / 3
                if resblock2:                                                 # x <- conv_d(lrelu x) + x
                    launch(f'{name}.convs.{p}', src, dst, c, c, k, d, 1, 1, acc, scale, d * h, r=src)
                elif c <= 64 and not training:
                    launch(f'{name}.convs1.{p}', src, dst, c, c, k, d, 1, 1, acc, scale, d * h + h, kind='pair', layer2=f'{name}.convs2.{p}')
                else:
                    mid = tensor(f'{name}.mid{p}', scale, c, 4)            # training keeps every mid_p: the name carries p
                    launch(f'{name}.convs1.{p}', src, mid, c, c, k, d, 1, 1, 0, scale, d * h)
                    launch(f'{name}.convs2.{p}', mid, dst, c, c, k, 1, 1, 1, acc, scale, h, r=src)
                src = dst
        x = total
    launch('conv_post', x, 'audio', c, 1, 7, 1, 1, 1, 0, scale, 3, kind='post')
    return GeneratorLaunches(T, L)


def _issue(L, ln, packs, x, y, r, frames, B, N, bf16, window, st):
    """One launch of ``generator_launches`` as its call into the library.  ``x``, ``y``, ``r`` (None without a residual): where the
    launch's tensors are, each as (pointer, batch stride, row stride, channel stride, ring mask -- 0: not a ring); ``N``: the rows of
    x; ``window``: None for the whole tensors, or (cursor, step, lag) for the windowed entry point of the same name."""
    (X, sxb, sxn, sxc, mx), (Y, syb, _, _, my) = x, y
    kind, whole, masks = ln['kind'], window is None, (mx, my)
    w, b = packs[ln['layer']]
    if kind == 'conv':
        R, srb, _, _, mr = (None, ln['cout'], 0, 0, 0) if r is None else r
        args = (X, sxb, sxn, sxc, w.data_ptr(), b.data_ptr(), Y, syb, R) + (() if whole else (srb,)) + (
            frames, ln['scale'], B, N, ln['cin'], ln['cout'], ln['taps'], ln['dil'], ln['up'], ln['lrelu'], ln['acc'], bf16)
        masks = (mx, my, mr)
    elif kind == 'post':                                  # y: the audio, its batch stride the row's samples
        args = (X, sxb, w.data_ptr(), b.data_ptr(), Y, syb, frames, ln['scale'], B, N, syb, ln['cin'])
    else:                                                 # 'pair' and 'chain': two layers, the second dilation the chain's alone
        w2, b2 = packs[ln['layer2']]
        args = (X, sxb, w.data_ptr(), b.data_ptr(), w2.data_ptr(), b2.data_ptr(), Y) + (() if whole else (syb,)) + (
            frames, ln['scale'], B, N, ln['cin'], ln['taps'], ln['dil']) + ((ln['dil2'],) if kind == 'chain' else ()) + (ln['acc'], bf16)
    entry = 'dx_voc_post_c' if kind == 'post' else 'dx_voc_' + kind
    tail = () if whole else (*window, *masks)
    getattr(L, entry + ('_win' if tail else ''))(*args, *tail, st)


# ---- the streaming plan (host only) ----------------------------------------------------------------------------------------------
class StreamPlan:
    """What ``stream_plan`` returns.  ``tensors``: ``generator_launches``' with 'lag', 'left' and 'ring' added; ``launches``: the chunk's
    launches in order, ``generator_launches``' with 'step' = chunk_frames * scale and 'lag' added; ``lookahead``: mel frames past a
    chunk's own that the chunk reads."""

    def __init__(self, chunk_frames, tensors, launches, lookahead):
        self.chunk_frames, self.tensors, self.launches, self.lookahead = chunk_frames, tensors, launches, lookahead

    def ring_bytes(self, batch=1):
        return sum(batch * t['ring'] * t['channels'] * 4 for t in self.tensors.values())


def stream_plan(config=None, chunk_frames=32, precision='f32') -> StreamPlan:
    """The schedule of the chunked generator: ``generator_launches(config, precision)`` with a lag for every tensor and launch and a ring
    for every tensor.  After chunk c, rows [0, min(len, (c + 1) F scale + lag)) of a tensor exist; chunk c
    computes rows [c F scale + lag (0 for c = 0), (c + 1) F scale + lag) of it, F = chunk_frames.

    Lags come from walking the generator backwards from conv_post's output (lag 0): a tensor's lag is the largest, over the launches that
    read it, of that launch's own lag (in the tensor's rows) plus its right reach -- dil (k - 1) / 2 for a dilated conv, that plus
    (k - 1) / 2 for a fused pair, (d1 + d2) (k - 1) / 2 for a fused ResBlock2 chain, 3 for conv_post, 1 for a polyphase transposed conv (output row s up + r reads input rows s + base_r and
    s + base_r + 1, base_r in {-1, 0}), whose output lag is rounded up to a multiple of up so that its window is whole input rows.  A
    residual and an accumulated output are read at the launch's own rows.  Row n of a tensor lives at slot n & (ring - 1); the ring is
    the power of two that holds the chunk-0 window (F scale + lag) and, for every reader, F scale + (lag - reader's lag) + the reader's
    left reach: what is resident between the oldest row a reader of chunk c still needs and the newest row chunk c has written."""
    F = int(chunk_frames)
    if F < 1:
        raise ValueError(f'stream_plan: chunk_frames must be >= 1, got {chunk_frames}')
    generator = generator_launches(config, precision)
    T = {name: dict(t, lag=0, left=0, ring=0) for name, t in generator.tensors.items()}
    L = [dict(ln) for ln in generator.launches]              # copies: the pass below writes 'lag' and 'step' into them
    lookahead = 0
    for ln in reversed(L):                                  # every reader of a tensor comes after its writer: lags settle backwards
        up = ln['up']
        if ln['y'] != 'audio':
            T[ln['y']]['lag'] = -(-T[ln['y']]['lag'] // up) * up
        ln['lag'] = 0 if ln['y'] == 'audio' else T[ln['y']]['lag'] // up
        ln['step'] = F * ln['scale']
        if ln['x'] == 'mel':
            lookahead = ln['lag'] + ln['right']
        else:
            tx = T[ln['x']]
            tx['lag'], tx['left'] = max(tx['lag'], ln['lag'] + ln['right']), max(tx['left'], ln['left'])
        if ln['r'] is not None:
            T[ln['r']]['lag'] = max(T[ln['r']]['lag'], ln['lag'])
    for name, t in T.items():
        need = F * t['scale'] + t['lag']
        for ln in L:
            if ln['x'] == name:
                need = max(need, F * t['scale'] + t['lag'] - ln['lag'] + ln['left'])
            if ln['r'] == name or (ln['y'] == name and ln['acc']):
                need = max(need, F * t['scale'] + t['lag'] - ln['lag'] * ln['up'])
        t['ring'] = 1 << (need - 1).bit_length()
    return StreamPlan(F, T, L, lookahead)


class _WNConv(nn.Module):
    """Parameters of one weight-normed (transposed) convolution, named as torch.nn.utils.weight_norm names them."""

    def __init__(self, w_shape, n_bias):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(n_bias))
        self.weight_g = nn.Parameter(torch.ones(w_shape[0], 1, 1))
        self.weight_v = nn.Parameter(torch.zeros(*w_shape))


class _ResBlock1(nn.Module):
    def __init__(self, channels, k, dilations):
        super().__init__()
        self.convs1 = nn.ModuleList([_WNConv((channels, channels, k), channels) for _ in dilations])
        self.convs2 = nn.ModuleList([_WNConv((channels, channels, k), channels) for _ in dilations])


class _ResBlock2(nn.Module):
    def __init__(self, channels, k, dilations):
        super().__init__()
        self.convs = nn.ModuleList([_WNConv((channels, channels, k), channels) for _ in dilations])


class HiFiGANGenerator(nn.Module):
    """The reference generator (weight-normed keys and shapes).  ``generator(x)``, x a (B, 80, T) fp32 mel on the device -> (B, 1, 256 T),
    the reference's signature; ``lengths``: optional frame counts per row, ``infer_batch``'s semantics (samples at or past 256
    lengths[b] are 0, and constant).  With grad mode on and a parameter that requires grad, the forward runs the training launch list
    and ``backward()`` leaves ``.grad`` on every weight_g, weight_v and bias (vocoder_train.py: f32 operands only, once per forward, no
    gradient to the mel); otherwise it is ``HiFiGanVocoder(state_dict).infer_batch``, bit for bit."""

    def __init__(self, config=None, precision='f32'):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f'HiFiGANGenerator: precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        self.config = check_config(config)
        self.precision = precision
        self._inference = None                                  # (parameter versions, the HiFiGanVocoder of those weights)
        c0 = self.config['upsample_initial_channel']
        self.conv_pre = _WNConv((c0, self.config['model_in_dim'], 7), c0)
        self.ups = nn.ModuleList([_WNConv((c0 >> i, c0 >> (i + 1), k), c0 >> (i + 1))
                                  for i, k in enumerate(self.config['upsample_kernel_sizes'])])
        block = _ResBlock2 if str(self.config['resblock']) == '2' else _ResBlock1
        widths = stage_widths(self.config, padded=False)        # the checkpoint's own widths: padding happens after folding
        self.resblocks = nn.ModuleList([block(c, k, d) for c in widths
                                        for k, d in zip(self.config['resblock_kernel_sizes'], self.config['resblock_dilation_sizes'])])
        self.conv_post = _WNConv((1, widths[-1], 7), 1)

    def layer_names(self):
        return [n[:-len('.bias')] for n, _ in self.named_parameters() if n.endswith('.bias')]

    def folded(self) -> dict:
        """-> {layer: (weight, bias)} with weight norm folded (CPU fp32)."""
        return fold_state_dict({k: v.detach().cpu() for k, v in self.state_dict().items()}, self.layer_names())

    def forward(self, x, lengths=None):
        from .vocoder_train import generator_forward
        return generator_forward(self, x, lengths)


def fold_state_dict(state: dict, layers) -> dict:
    """Generator state dict, weight-normed (``weight_g`` / ``weight_v``) or already folded (``weight``) -> {layer: (weight, bias)}."""
    out = {}
    for name in layers:
        if name + '.weight' in state:
            w = state[name + '.weight'].float()
        elif name + '.weight_v' in state and name + '.weight_g' in state:
            w = torch._weight_norm(state[name + '.weight_v'].float(), state[name + '.weight_g'].float(), 0)
        else:
            raise KeyError(f'generator checkpoint has no weight for {name!r}')
        if name + '.bias' not in state:
            raise KeyError(f'generator checkpoint has no bias for {name!r}')
        out[name] = (w.detach().cpu().contiguous(), state[name + '.bias'].float().detach().cpu().contiguous())
    return out


def _checkpoint_state(checkpoint) -> dict:
    """The generator state dict from any form the reference's _load_generator accepts: {'generator': sd}, {'state_dict': sd}, sd."""
    if isinstance(checkpoint, (str, os.PathLike)):
        checkpoint = torch.load(checkpoint, map_location='cpu')
    if not isinstance(checkpoint, dict):
        raise TypeError(f'a generator checkpoint is a dict or a state dict, got {type(checkpoint).__name__}')
    for wrapper in ('generator', 'state_dict'):         # a training checkpoint nests the generator's weights under one of these
        if wrapper in checkpoint:
            return checkpoint[wrapper]
    return checkpoint


def config_from_state(state: dict) -> dict:
    """The configuration a generator state dict was saved under, from conv_pre's width, the number of ``ups`` and the ResBlock kind
    (``convs1`` / ``convs2``: ResBlock1; ``convs``: ResBlock2); NotImplementedError if they match none of V1, V2, V3."""
    if 'conv_pre.bias' not in state:
        raise KeyError("generator checkpoint has no bias for 'conv_pre'")
    width = int(state['conv_pre.bias'].shape[0])
    n_ups = len({k.split('.')[1] for k in state if k.startswith('ups.')})
    kind = '2' if any(k.startswith('resblocks.0.convs.') for k in state) else '1'
    for make in CONFIGS.values():
        cfg = make()
        if (cfg['upsample_initial_channel'], len(cfg['upsample_rates']), cfg['resblock']) == (width, n_ups, kind):
            return cfg
    raise NotImplementedError(f'a generator of {width} channels, {n_ups} upsampling stages and ResBlock{kind} is none of HiFi-GAN V1 '
                              f'(512, 4, ResBlock1), V2 (128, 4, ResBlock1), V3 (256, 3, ResBlock2)')


class HiFiGanVocoder:
    """Drop-in for the reference ``HiFiGanVocoder`` on gfx950.  ``checkpoint_path``: a local generator checkpoint (or its loaded dict);
    ``config``: None (V1) or one of ``v1_config()``, ``v2_config()``, ``v3_config()``.  ``from_checkpoint`` reads it off the weights."""

    @classmethod
    def from_checkpoint(cls, checkpoint, device='cuda', precision='f32'):
        """A vocoder for a V1, V2 or V3 checkpoint (a local path or its loaded dict), the configuration taken from the shapes."""
        if checkpoint is None:
            raise ValueError('from_checkpoint: checkpoint_path is required (a local HiFi-GAN generator checkpoint)')
        state = _checkpoint_state(checkpoint)
        vocoder = cls(state, config=config_from_state(state), device=device, precision=precision)
        vocoder.checkpoint_path = checkpoint
        return vocoder

    def __init__(self, checkpoint_path=None, config=None, device='cuda', precision='f32'):
        if checkpoint_path is None:
            raise ValueError('HiFiGanVocoder: checkpoint_path is required (a local HiFi-GAN generator checkpoint); '
                             'this package never downloads one')
        if precision not in PRECISIONS:
            raise ValueError(f'HiFiGanVocoder: precision must be one of {sorted(PRECISIONS)}, got {precision!r}')
        generator = HiFiGANGenerator(config)
        self.config = generator.config
        self.checkpoint_path = checkpoint_path
        self.precision = precision
        self.topology = generator_launches(self.config, precision)     # what infer_batch issues; stream_plan schedules the same list
        self.device = torch.device(device)
        state = _checkpoint_state(checkpoint_path)
        layers = generator.layer_names()
        self.weights = fold_state_dict(state, layers)          # {layer: (folded weight, bias)}, CPU fp32: what the kernels run
        # ``generator``: the checkpoint's weight-normed parameters (CPU, frozen: ``infer`` / ``infer_batch`` are this object's
        # forward).  None for a checkpoint that is already folded: there are no weight_g / weight_v to hold.
        self.generator = None
        if all(n + '.weight_v' in state for n in layers):
            generator.load_state_dict(state, strict=True)
            self.generator = generator.eval().requires_grad_(False)
        self._packs = None

    # -- device-side weights -------------------------------------------------------------------------------------------------
    def _pack(self, w, up=1):
        """folded weight -> dx_voc_pack operand (uint8 device buffer)."""
        bf16 = PRECISIONS[self.precision]
        if up > 1:
            cin, cout, _ = w.shape
            taps = 2
        else:
            cout, cin, taps = w.shape
        return _packed('voc', w.to(self.device).contiguous(), (cout, cin, taps, up, bf16), self.device)

    def _device_weights(self):
        if self._packs is None:
            if self.device.type != 'cuda':
                raise RuntimeError('HiFiGanVocoder runs on the GPU (gfx950 HIP kernels); there is no CPU path')
            dev = lambda t: t.to(self.device).contiguous()
            P = {}
            weights = pad_folded_weights(self.weights, self.config)     # a stage narrower than 16 channels runs zero-padded to 16
            w, b = weights['conv_pre']
            P['conv_pre'] = (self._pack(w), dev(b))
            for i, u in enumerate(self.config['upsample_rates']):
                w, b = weights[f'ups.{i}']
                P[f'ups.{i}'] = (self._pack(w, up=u), dev(b))
            for name, (w, b) in weights.items():
                if name.startswith('resblocks.'):
                    P[name] = (self._pack(w), dev(b))
            w, b = weights['conv_post']
            P['conv_post'] = (dev(w), dev(b))
            self._packs = P
        return self._packs

    # -- reference contract ----------------------------------------------------------------------------------------------------
    def infer(self, mel_spec):
        """(80, T) or (1, 80, T) mel (numpy, tensor or nested list) -> numpy waveform clipped to [-1, 1], as the reference's infer."""
        mel = mel_spec.detach().float() if torch.is_tensor(mel_spec) else torch.as_tensor(np.asarray(mel_spec, dtype=np.float32))
        if mel.dim() == 3:
            if mel.shape[0] != 1:
                raise ValueError(f'infer vocodes one utterance, got a batch of {mel.shape[0]} mels: use infer_batch')
            mel = mel[0]
        if mel.dim() != 2:
            raise ValueError(f'infer takes a ({N_MELS}, T) or (1, {N_MELS}, T) mel, got shape {tuple(mel.shape)}')
        mel = mel[None]
        mel = mel.to(self.device).contiguous()
        with torch.no_grad():
            audio, _ = self.infer_batch(mel, [mel.shape[-1]])
            audio = audio.squeeze().cpu().numpy()
        return np.clip(audio, -1.0, 1.0)

    # -- batched form ----------------------------------------------------------------------------------------------------------
    def _check_batch(self, who, mels, lengths):
        """-> (mels fp32 contiguous, host frame counts clamped to [0, T], the same on the device as int32, sample lengths)."""
        if mels.dim() != 3 or mels.shape[1] != self.config['model_in_dim']:
            raise ValueError(f'{who}: mels must be (B, {self.config["model_in_dim"]}, T_max), got {tuple(mels.shape)}')
        if mels.device != self.device and not (self.device.index is None and mels.device.type == self.device.type):
            raise ValueError(f'{who}: mels are on {mels.device}, the vocoder on {self.device}')
        mels = mels.float().contiguous()
        B, _, T = mels.shape
        dev = mels.device
        if torch.is_tensor(lengths):
            host = lengths.tolist()                                       # the one device-to-host copy (sizing only)
            frames = lengths.to(device=dev, dtype=torch.int32).clamp(0, T).contiguous()
            sample_lengths = frames.to(torch.long) * HOP
        else:
            host = [int(v) for v in lengths]
            frames = torch.tensor(host, dtype=torch.int32).clamp(0, T).to(dev)
            sample_lengths = [min(max(v, 0), T) * HOP for v in host]
        if len(host) != B:
            raise ValueError(f'{who}: {len(host)} lengths for a batch of {B}')
        return mels, [min(max(int(v), 0), T) for v in host], frames, sample_lengths

    def stream(self, mels, lengths, chunk_frames=32, use_graph=True, clone=True):
        """``infer_batch``'s mels and lengths -> a ``VocoderStream``: an iterator of ``len(stream)`` = max(1, ceil(max(lengths) /
        chunk_frames)) steps, each yielding (audio (B, 256 chunk_frames) fp32 on the device, valid (B,) int64 on the device).  Step c
        holds samples [256 c chunk_frames, 256 (c + 1) chunk_frames) of every row, bit for bit what ``infer_batch`` writes there;
        ``valid`` counts those that belong to the row (0 once the row has ended; the rest of its chunk is 0).  Every step runs the same
        launches (the ``len(generator_launches(config, precision))`` of the generator and the cursor's advance) on ring buffers whose
        size depends on chunk_frames and B alone (``stream.workspace_bytes``); with ``use_graph``
        they are captured once, while the second chunk is due, and replayed from then on.  ``clone=False`` yields the stream's own
        buffer, overwritten by the next step.  The mel is read in place until the last step: leave it unchanged meanwhile."""
        return VocoderStream(self, mels, lengths, chunk_frames, use_graph, clone)

    def infer_batch(self, mels, lengths, max_workspace_bytes=DEFAULT_WORKSPACE_BYTES):
        """mels (B, 80, T_max) fp32 on the device; lengths: B frame counts (host ints, or a device tensor such as GraphedSynthesizer's
        out_lens: one small device-to-host copy sizes the work).  -> (audio (B, 256 T_max) fp32 on the device, sample_lengths).
        Row b is bitwise ``mel[b, :, :lengths[b]]`` vocoded alone; samples at or past 256 lengths[b] are 0.  max_workspace_bytes
        bounds the activation workspace: the batch then runs in chunks of consecutive utterances (bitwise the same result).  A chunk
        of b utterances whose longest has n frames takes b * n * workspace_bytes_per_frame(config) (V1 and V3: 160 KB per frame, V2: 80 KB;
        sized by the LONGEST row: 2.2 GB for 16 rows of 850 frames of V1); one utterance longer than the bound still runs, alone.  None: no bound, one chunk.
        Nothing is returned before the last sample exists: ``stream`` yields the same samples chunk by chunk, in a workspace that does
        not grow with the length."""
        mels, host, frames, sample_lengths = self._check_batch('infer_batch', mels, lengths)
        B, n_mel, T = mels.shape
        dev = mels.device
        P = self._device_weights()
        audio = torch.empty(B, T * HOP, dtype=torch.float32, device=dev)
        per_frame = workspace_bytes_per_frame(self.config)
        b0 = 0
        while b0 < B:
            b1, n = b0 + 1, max(1, host[b0])
            while b1 < B:
                n2 = max(n, host[b1])
                if max_workspace_bytes is not None and (b1 + 1 - b0) * n2 * per_frame > max_workspace_bytes:
                    break
                b1, n = b1 + 1, n2
            self._run(P, mels, frames, audio, b0, b1, n)
            b0 = b1
        return audio, sample_lengths

    def _run(self, P, mels, frames, audio, b0, b1, N):
        """Utterances b0 .. b1-1 with N frames of work each (N >= their lengths): the ``len(generator_launches(config, precision))``
        launches, every tensor whole ((B, N scale, channels), channels last) in its slot of a workspace of five."""
        L, st = lib(), _stream(mels.device)
        B, n_mel, T = b1 - b0, mels.shape[1], mels.shape[2]
        ws = torch.empty(5, B * N * (workspace_bytes_per_frame(self.config) // 20), dtype=torch.float32, device=mels.device)
        slots = [ws[i].data_ptr() for i in range(5)]
        at = {'mel': (mels.data_ptr() + 4 * b0 * n_mel * T, n_mel * T, 1, T, 0), 'audio': (audio.data_ptr() + 4 * b0 * T * HOP, T * HOP, 0, 0, 0), None: None}
        at.update((name, (slots[t['slot']], N * t['scale'] * t['channels'], t['channels'], 1, 0)) for name, t in self.topology.tensors.items())
        fr, bf16 = frames.data_ptr() + 4 * b0, PRECISIONS[self.precision]
        for ln in self.topology.launches:
            _issue(L, ln, P, at[ln['x']], at[ln['y']], at[ln['r']], fr, B, N * ln['scale'], bf16, None, st)


class VocoderStream:
    """One utterance batch being vocoded chunk by chunk (``HiFiGanVocoder.stream``).  It owns everything it touches -- the ring buffer
    of every tensor of ``stream_plan``, the device cursor the window kernels read the chunk index from, the chunk buffer and the
    captured graph -- so streams of one vocoder may be interleaved, and one that is dropped leaves nothing behind.
    ``workspace_bytes``: rings + chunk buffer + cursor; ``captures``: graphs captured so far (at most 1).  ``tail``: a callable given the
    chunk buffer inside every chunk, after conv_post and before the cursor advances (``SpeechSynthesizer.stream``'s PCM launch); it is
    captured with the chunk, so it may launch but not allocate."""

    def __init__(self, vocoder, mels, lengths, chunk_frames=32, use_graph=True, clone=True, tail=None):
        if int(chunk_frames) < 1:
            raise ValueError(f'stream: chunk_frames must be >= 1, got {chunk_frames}')
        self.mels, host, self.frames, _ = vocoder._check_batch('stream', mels, lengths)
        self.packs = vocoder._device_weights()
        self.plan = stream_plan(vocoder.config, int(chunk_frames), vocoder.precision)
        self.bf16 = PRECISIONS[vocoder.precision]
        self.use_graph, self.clone, self.tail = bool(use_graph), bool(clone), tail
        B, dev = self.mels.shape[0], self.mels.device
        self.chunk_samples = self.plan.chunk_frames * HOP
        self.n_chunks = max(1, -(-max(host) // self.plan.chunk_frames))
        self.rings = {name: torch.zeros(B, t['ring'], t['channels'], dtype=torch.float32, device=dev) for name, t in self.plan.tensors.items()}
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.audio = torch.zeros(B, self.chunk_samples, dtype=torch.float32, device=dev)
        self.workspace_bytes = self.plan.ring_bytes(B) + self.audio.numel() * 4 + 4
        n_mel, T = self.mels.shape[1:]
        # where _issue finds every tensor: the mel in place, the chunk buffer, its ring (row n at slot n & (ring - 1))
        self.at = {'mel': (self.mels.data_ptr(), n_mel * T, 1, T, 0), 'audio': (self.audio.data_ptr(), self.chunk_samples, 0, 0, 0), None: None}
        self.at.update((name, (self.rings[name].data_ptr(), t['ring'] * t['channels'], t['channels'], 1, t['ring'] - 1)) for name, t in self.plan.tensors.items())
        start = torch.arange(self.n_chunks, device=dev)[:, None] * self.chunk_samples
        self.valid = (self.frames.to(torch.long)[None, :] * HOP - start).clamp(0, self.chunk_samples)       # (chunks, B)
        self.graph, self.captures, self.done = None, 0, 0

    def __len__(self):
        return self.n_chunks

    def __iter__(self):
        return self

    def _launch(self):
        """The launches of one chunk, the same for every chunk: the window comes from the device cursor, which the last one advances."""
        L, st = lib(), _stream(self.mels.device)
        B, T = self.mels.shape[0], self.mels.shape[2]
        fr, cur, at = self.frames.data_ptr(), self.cursor.data_ptr(), self.at
        for ln in self.plan.launches:
            _issue(L, ln, self.packs, at[ln['x']], at[ln['y']], at[ln['r']], fr, B, T * ln['scale'], self.bf16, (cur, ln['step'], ln['lag']), st)
        if self.tail is not None:
            self.tail(self.audio)
        L.dx_voc_stream_advance(cur, st)

    def __next__(self):
        if self.done >= self.n_chunks:
            raise StopIteration
        with torch.no_grad():
            if self.graph is not None:
                self.graph.replay()
            elif self.use_graph and self.done == 1:       # chunk 0 ran eagerly (first audio as early as possible, and the warm-up)
                self.graph, self.captures = capture(self._launch)[0], self.captures + 1
                self.graph.replay()
            else:
                self._launch()
        valid = self.valid[self.done]
        self.done += 1
        return (self.audio.clone() if self.clone else self.audio), valid


def load_hifigan_vocoder(checkpoint_path=None, device=None, precision='f32'):
    """Drop-in for the reference's load_hifigan_vocoder (scripts/synthesize.py:380-382); ``checkpoint_path`` is required."""
    if device is None:
        device = 'cuda'
    return HiFiGanVocoder(checkpoint_path=checkpoint_path, config=DEFAULT_CONFIG, device=device, precision=precision)
