"""Float64 restatement of the fused pitch-predictor chain (csrc/dx_pitch.hip), the inputs of its exact and rounded test tiers, and the
planted errors that keep the checks honest (tests/test_pitch_exact_cpu.py tests this file; tests/test_pitch_exact_gpu.py uses it).

Two tiers.  EXACT: an integer-valued network whose every intermediate is a small integer, representable in bf16 and fp16 and summed far
below 2^24, so the device must equal float64 bit for bit in any summation order.  ROUNDED: a dense random network against float64
arithmetic that rounds where the kernel rounds; the bar is 4 x the restatement's own spread when its sums are formed in fp32 in other
orders (``FLOOR``, measured on the CPU with no device result involved).

Rounding points of the kernels (pitch_fwd_kernel / pitch_bwd_kernel):
  forward   mel -> 16 bit (RNE), zero outside [0, min(rows_exist, T)); W0..W2 as the pack rounds them (RNE); v = conv + bias, sign = v > 0;
            x = relu(v) * scale + shift in fp32 -> 16 bit, zero outside the existing frames; pp = conv(x2, fp32 w3) + b3
  backward  conv^T(w3)(dpp) in fp32 x scale2 x mask2 -> 16 bit; conv^T(W2) x scale1 x mask1 -> 16 bit; conv^T(W1) x scale0 x mask0 -> 16 bit;
            conv^T(W0) in fp32, added to dmel; frames at or past min(rows_exist, T) are absent throughout
"""
import torch

H16 = {'bf16': torch.bfloat16, 'fp16': torch.float16}
TOK = 122                    # PC_TOK: output frames per tile
MAX_B = 1000                 # PC_MAX_B
MAX_GRID = 256               # workgroups of a launch; more tiles than that are strided over

# ---- the rounded tier's noise floor -------------------------------------------------------------------------------------------------
# Largest |variant - float64| over the fp32 summation orders ``ORDERS`` and the rounded tier's two cases, measured by ``measure_floor``
# on the CPU (test_pitch_exact_cpu.py re-measures and requires constant / measurement in [1, 2]).  Bars are BAR_FACTOR x these.
ORDERS = ((2, False), (4, False), (1, True))     # (accumulators the K range is cut into, taps walked in reverse)
BAR_FACTOR = 4.0
FLOOR = {
    'bf16': {'pp_max': 8.3e-3, 'pp_mean': 3.2e-5, 'dmel_max': 1.13e-3, 'dmel_mean': 2.1e-6},     # measured 6.63e-3, 2.53e-5, 9.04e-4, 1.67e-6
    'fp16': {'pp_max': 1.9e-3, 'pp_mean': 1.9e-5, 'dmel_max': 1.35e-4, 'dmel_mean': 4.9e-7},     # measured 1.54e-3, 1.54e-5, 1.09e-4, 3.95e-7
}
MAX_MASK_EXCLUDED = 0.01     # share of mask bits that may sit within tau of zero


def bar(mode, figure):
    return BAR_FACTOR * FLOOR[mode][figure]


# ---------------------------------------------------------------------------------------------------------------------------------------
# rounding, masks, small tools
# ---------------------------------------------------------------------------------------------------------------------------------------
def rnd(t, mode, trunc=False):
    """float64 -> fp32 -> the mode's 16-bit type (round to nearest even) -> float64; ``mode`` None: nothing is rounded.
    ``trunc`` (a planted error): the fp32 value's low 16 bits are cut off instead (bf16 only)."""
    if mode is None:
        return t.double()
    f = t.float()
    if trunc:
        assert mode == 'bf16'
        return (f.contiguous().view(torch.int32) & -65536).view(torch.float32).double()
    return f.to(H16[mode]).double()


def exist_mask(B, T, rows_exist, device):
    """(B, T) bool: frame n < min(rows_exist[b], T)"""
    n = torch.arange(T, device=device)[None, :]
    if rows_exist is None:
        return (n < T).expand(B, T)
    return n < torch.as_tensor(rows_exist, device=device).long()[:, None].clamp(max=T)


def valid_mask(lens, T, device, extra=0):
    """(B, T) bool: n < lens[b] + extra"""
    return torch.arange(T, device=device)[None, :] < (torch.as_tensor(lens, device=device).long()[:, None] + extra)


def decode_masks(masks):
    """(B, T, 3, 8) uint32 words (stored as int32) -> (B, T, 3, 256) bool: bit c % 32 of word c // 32 is channel c"""
    w = masks.to(torch.int64)[..., None]
    bits = (w >> torch.arange(32, device=masks.device)) & 1
    return bits.bool().reshape(*masks.shape[:-1], 256)


def encode_masks(signs):
    """(B, T, 3, 256) bool -> (B, T, 3, 8) int32, the inverse of ``decode_masks``"""
    b = signs.reshape(*signs.shape[:-1], 8, 32).to(torch.int64)
    w = (b << torch.arange(32, device=signs.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def signs_of(masks):
    """(B, T, 3, 8) words -> the three (B, 256, T) bool tensors ``chain64_bwd`` takes"""
    d = decode_masks(masks)
    return [d[:, :, l, :].transpose(1, 2) for l in range(3)]


def bits_equal(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


def tiles(lens, T):
    """[(b, n0)] in launch order: ceil(min(len, T) / 122) tiles per utterance"""
    return [(b, k * TOK) for b, n in enumerate(lens) for k in range((min(max(int(n), 0), T) + TOK - 1) // TOK)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the convolution, in float64 or as fp32 partial sums in a stated order
# ---------------------------------------------------------------------------------------------------------------------------------------
def _shift(x, s):
    """out[..., n] = x[..., n + s], zero outside"""
    if s == 0:
        return x
    out = torch.zeros_like(x)
    T = x.shape[-1]
    if abs(s) < T:
        if s > 0:
            out[..., :T - s] = x[..., s:]
        else:
            out[..., -s:] = x[..., :T + s]
    return out


KSTEP = 32                   # input channels per MFMA K step: the accumulator is rounded to fp32 once per step at the least


def conv(x, w, order=None, bias=None):
    """'same' k = 3 convolution of x (B, Cin, T) with w (Cout, Cin, 3), both float64: y[n] = sum_t w[:, :, t] x[n + t - 1] (+ bias).
    ``order`` None: float64 throughout.  ``order`` = (parts, reverse): an fp32 accumulation at the granularity of the kernels' K steps.
    The product sum of each (tap, 32-channel block) is formed in float64 and rounded to fp32 (one MFMA step: what happens inside it is
    not modelled), and added to an fp32 accumulator tap-major, block-minor, as pc_mfma_pass walks them; ``parts`` > 1 cuts the blocks
    into that many accumulators that are added up afterwards (split K); ``reverse`` walks the taps backwards; the bias comes last."""
    assert x.dtype == torch.float64 and w.dtype == torch.float64
    K = w.shape[1]
    if order is None:
        y = sum(torch.einsum('oc,bcn->bon', w[:, :, t], _shift(x, t - 1)) for t in range(3))
        return y if bias is None else y + bias.double()[None, :, None]
    parts, reverse = order
    blocks = [(lo, min(lo + KSTEP, K)) for lo in range(0, K, KSTEP)]
    edges = [round(i * len(blocks) / parts) for i in range(parts + 1)]
    xs = [_shift(x, t - 1) for t in range(3)]
    total = None
    for a, b in zip(edges[:-1], edges[1:]):
        acc = None
        for t in (range(2, -1, -1) if reverse else range(3)):
            for lo, hi in blocks[a:b]:
                p = torch.einsum('oc,bcn->bon', w[:, lo:hi, t], xs[t][:, lo:hi]).float()
                acc = p if acc is None else acc + p
        if acc is not None:
            total = acc if total is None else total + acc
    if bias is not None:
        total = total + bias.float()[None, :, None]
    return total.double()


def transposed(w):
    """the weight of the input-gradient convolution: channel axes swapped, taps flipped (dx[m] = sum_t w[:, :, t]^T dy[m - t + 1])"""
    return w.transpose(0, 1).flip(2).contiguous()


def _affine(v, scale, shift, order):
    """relu(v) * scale + shift: float64 (``rnd`` takes it to fp32 on the way to 16 bit), or the kernel's two fp32 operations"""
    r = v.clamp_min(0)
    if order is None:
        return r * scale.double()[None, :, None] + shift.double()[None, :, None]
    return r.float() * scale.float()[None, :, None] + shift.float()[None, :, None]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------------------------
def chain64(mel, layers, mode, lens, rows_exist=None, order=None, plant=None):
    """The forward.  mel (B, M, T); ``layers``: the list ``fold_pitch_predictor`` produces ('w', 'b', 'scale', 'shift'; the last entry
    'w' (4, 256, 3) with row 0 real, 'b3').  ``mode``: 'bf16' / 'fp16' / None (nothing rounded).  Returns pp (B, T) and the three
    (B, 256, T) pre-activations, all float64, on every frame; the kernel writes pp on frames n < lens[b] only (``lens`` otherwise
    matters to the planted errors alone, which name tiles).  ``plant``: see ``PLANTS``."""
    B, M, T = mel.shape
    dev = mel.device
    ex = exist_mask(B, T, rows_exist, dev)[:, None, :]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    trunc = plant == 'trunc'
    x = torch.where(ex, rnd(mel, mode, trunc), zero)
    pre = []
    for l in range(3):
        w = rnd(layers[l]['w'], mode)
        if plant == 'drop_tap' and l == 1:
            w = w.clone()                    # one tap of one 32-channel K step, for one 16-row block: the block after (48, 96, 2) in
            blocks = [(r, k, t) for t in (2, 0, 1) for r in range(48, 256, 16) for k in range(96, 256, 32)]      # which a weight is nonzero
            r, k, t = next(b for b in blocks if bool(w[b[0]:b[0] + 16, b[1]:b[1] + 32, b[2]].any()))
            w[r:r + 16, k:k + 32, t] = 0
        v = conv(x, w, order, layers[l]['b'])
        pre.append(v)
        x = torch.where(ex, rnd(_affine(v, layers[l]['scale'], layers[l]['shift'], order), mode, trunc), zero)
    pp = conv(x, layers[3]['w'][:1].double(), order)[:, 0]
    pp = (pp.float() + float(layers[3]['b3'])).double() if order is not None else pp + float(layers[3]['b3'])
    if plant in ('halo', 'tile_off'):
        tl = [t for t in tiles(lens, T) if t[1] > 0]
        assert tl, 'these planted errors need an utterance of more than one tile'
        b, n0 = max(tl, key=lambda t: min(int(lens[t[0]]), T) - t[1])       # the later tile with the most frames below the length
        n1 = min(n0 + TOK, T)
        if plant == 'halo':                  # frame n0 - 1 (window row 3) missing from this tile's window: a zero where the mel is not
            m2 = mel[b:b + 1].clone()
            m2[:, :, n0 - 1] = 0
            re_b = None if rows_exist is None else [int(rows_exist[b])]
            pp_t, _ = chain64(m2, layers, mode, [lens[b]], re_b, order)
            pp = pp.clone()
            pp[b, n0:n1] = pp_t[0, n0:n1]
        else:                                # the tile's window starts one frame late
            sh = _shift(pp[b], 1)
            pp = pp.clone()
            pp[b, n0:n1] = sh[n0:n1]
    return pp, pre


def signs64(pre, plant=None):
    """the ReLU sign bits of float64 pre-activations: strictly positive"""
    return [(v >= 0) if plant == 'ge' else (v > 0) for v in pre]


def chain64_bwd(dpp, signs, layers, mode, rows_exist=None, order=None, plant=None):
    """The backward, linear in dpp (B, T) given the three (B, 256, T) bool sign tensors.  Returns d(sum pp * dpp) / d(mel) (B, M, T)
    float64 on every frame; the kernel adds it to dmel on frames n < lens[b] and expects dpp to be zero at and past lens[b]."""
    B, T = dpp.shape
    dev = dpp.device
    ex = exist_mask(B, T, rows_exist, dev)[:, None, :]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    trunc = plant == 'trunc'
    if plant == 'mask_word':                 # layer 1's words taken from the neighbouring channel group
        s1 = signs[1].reshape(B, 8, 32, T)[:, [1, 0, 3, 2, 5, 4, 7, 6]].reshape(B, 256, T)
        signs = [signs[0], s1, signs[2]]
    g = torch.where(ex, dpp.double()[:, None, :], zero)
    d = conv(g, transposed(layers[3]['w'][:1].double()), order)
    for l in (2, 1, 0):
        s = layers[l]['scale']
        d = d * s.double()[None, :, None] if order is None else d.float() * s.float()[None, :, None]
        d = torch.where(ex & signs[l], rnd(d, mode, trunc), zero)
        d = conv(d, transposed(rnd(layers[l]['w'], mode)), order)
    return d


def add_base(base, grad, lens, order=None):
    """what the backward launch leaves in dmel: base + gradient on frames n < lens[b], the base elsewhere; float64, or (``order``) the
    kernel's fp32 addition"""
    B, M, T = base.shape
    v = valid_mask(lens, T, base.device)[:, None, :]
    s = (base.float() + grad.float()).double() if order is not None else base.double() + grad
    return torch.where(v, s, base.double())


PLANTS = ('halo', 'trunc', 'drop_tap', 'mask_word', 'tile_off', 'ge')


# ---------------------------------------------------------------------------------------------------------------------------------------
# the integer network (exact tier)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _sparse_pm1(g, rows, cols, nnz):
    """(rows, cols): +-1 at ``nnz`` random positions per row"""
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:nnz]
        w[r, idx] = _randint(g, 0, 1, (nnz,)) * 2 - 1
    return w


def integer_layers(M=80, seed=0, device='cpu'):
    """A layer list with the keys of ``fold_pitch_predictor`` (without the packs), every number a small integer: weights of layers 0..2
    +-1 at 4 positions per output channel over (Cin, 3), biases in [-2, 2], scale +-1, shift in {-1, 0, 1}, w3 +-1 at every position (a
    sparse w3 leaves the gradient of a one-frame utterance, where only the centre taps act, almost empty), b3 = 1."""
    g = torch.Generator().manual_seed(1000 + seed)
    layers = []
    for cin in (M, 256, 256):
        w = _sparse_pm1(g, 256, cin * 3, 4).reshape(256, cin, 3)
        layer = {'w': w, 'b': _randint(g, -2, 2, (256,)), 'scale': _randint(g, 0, 1, (256,)) * 2 - 1, 'shift': _randint(g, -1, 1, (256,))}
        layer['zeros'] = torch.zeros(256)
        layers.append(layer)
    w3 = torch.zeros(4, 768)
    w3[0] = _randint(g, 0, 1, (768,)) * 2 - 1
    layers.append({'w': w3.reshape(4, 256, 3), 'b': torch.tensor([1., 0., 0., 0.]), 'scale': None, 'shift': None, 'b3': 1.0})
    return [{k: (v.to(device).contiguous() if torch.is_tensor(v) else v) for k, v in l.items()} for l in layers]


# name -> (M, T, lens, rows_exist): the smallest shapes that reach each edge of the launch
EXACT_CASES = {
    'edges': (80, 300, [1, 2, 3, 4, 5, 118, 121, 122, 123, 126, 130, 243, 244, 245, 300, 0], None),
    'many': (80, 9, [0 if b % 16 == 7 else 1 + b % 9 for b in range(320)], None),       # 300 tiles on 256 workgroups, five 64-lane prefix blocks
    'width72': (72, 130, [130, 123, 7], None),
    'width96': (96, 130, [130, 123, 7], None),
    'rows_exist': (80, 300, [250, 122, 122, 3], [250, 130, 122, 5]),
    'one_frame': (80, 1, [1, 1, 0], None),
    'max_batch': (80, 3, [(b * 7) % 4 for b in range(MAX_B)], None),
}


def exact_inputs(name, seed=0, device='cpu'):
    """(layers, mel, dpp, base, lens, rows_exist) of one exact-tier case: mel integers in [-2, 2] on every stored frame (past the
    lengths too), dpp in {-1, 0, 1} and zero at and past the length, base (what dmel holds before the launch) integers in [-8, 8]."""
    M, T, lens, rows_exist = EXACT_CASES[name]
    B = len(lens)
    g = torch.Generator().manual_seed(2000 + seed)
    mel = _randint(g, -2, 2, (B, M, T))
    dpp = _randint(g, -1, 1, (B, T)) * valid_mask(lens, T, 'cpu')
    base = _randint(g, -8, 8, (B, M, T))
    return integer_layers(M, seed, device), mel.to(device), dpp.to(device), base.to(device), lens, rows_exist


def assert_integer(t, what, limit):
    """``t`` (float64) holds integers of magnitude <= limit: exact in the 16-bit types when limit <= 256, and any fp32 sum of them in
    any order is exact while the sum of magnitudes stays below 2^24 (it does by orders of magnitude: <= 768 terms of <= 256)"""
    assert bool((t == t.round()).all()), f'{what}: not integer-valued'
    m = float(t.abs().max()) if t.numel() else 0.0
    assert m <= limit, f'{what}: magnitude {m} > {limit}'
    return m


def exact_reference(layers, mel, dpp, base, lens, rows_exist):
    """float64 results of an exact-tier case and the proof that they are exact on the device: every tensor a kernel rounds is asserted
    to be unchanged by rounding to bf16 AND fp16 (integers <= 256), every fp32 sum to stay below 2^24.  Returns a dict: pp, pre (3),
    signs (3), grad, dmel (base + grad where n < len), stats."""
    outs = {}
    for mode in ('bf16', 'fp16'):
        pp, pre = chain64(mel, layers, mode, lens, rows_exist)
        sg = signs64(pre)
        grad = chain64_bwd(dpp, sg, layers, mode, rows_exist)
        outs[mode] = (pp, pre, sg, grad)
    pp0, pre0 = chain64(mel, layers, None, lens, rows_exist)
    sg0 = signs64(pre0)
    grad0 = chain64_bwd(dpp, sg0, layers, None, rows_exist)
    for mode in ('bf16', 'fp16'):                       # rounding changes nothing anywhere  <=>  the rounded chains equal the unrounded one
        pp, pre, sg, grad = outs[mode]
        assert torch.equal(pp, pp0) and torch.equal(grad, grad0) and all(torch.equal(a, b) for a, b in zip(pre, pre0)), mode
    B, M, T = mel.shape
    ex = exist_mask(B, T, rows_exist, mel.device)[:, None, :]
    # magnitudes: stored activations (16-bit) <= 256; the fp32 sums are of <= 768 such terms times +-1 weights, so < 2^18
    act = 0.0
    x = torch.where(ex, mel.double(), torch.zeros((), dtype=torch.float64, device=mel.device))
    assert_integer(x, 'mel', 256)
    for l in range(3):
        assert_integer(pre0[l], f'pre-activation {l}', 2 ** 24 / 1024)
        xl = pre0[l].clamp_min(0) * layers[l]['scale'].double()[None, :, None] + layers[l]['shift'].double()[None, :, None]
        act = max(act, assert_integer(torch.where(ex, xl, torch.zeros_like(xl)), f'activation {l}', 256))
        assert_integer(layers[l]['w'].double(), f'weight {l}', 1)
    assert_integer(pp0, 'pp', 2 ** 24 / 1024)
    # backward intermediates, re-derived stage by stage
    g = torch.where(ex, dpp.double()[:, None, :], torch.zeros((), dtype=torch.float64, device=mel.device))
    d = conv(g, transposed(layers[3]['w'][:1].double()))
    bwd = 0.0
    for l in (2, 1, 0):
        d = torch.where(ex & sg0[l], d * layers[l]['scale'].double()[None, :, None], torch.zeros_like(d))
        bwd = max(bwd, assert_integer(d, f'backward stage {l}', 256))
        d = conv(d, transposed(layers[l]['w'].double()))
    assert torch.equal(d, grad0)
    assert_integer(grad0, 'gradient', 2 ** 24 / 1024)
    dmel = add_base(base, grad0, lens, None)
    assert_integer(dmel, 'dmel', 2 ** 23)
    v3 = valid_mask(lens, T, mel.device)[:, None, :]
    nv = max(int(v3.sum()), 1)
    allpre = torch.stack(pre0)                           # (3, B, 256, T)
    vp = v3.expand_as(pre0[0])[None].expand_as(allpre)
    stats = {'act_max': act, 'bwd_max': bwd,
             'zero': float((allpre[vp] == 0).float().mean()) if nv else 0.0,
             'pos': float((allpre[vp] > 0).float().mean()) if nv else 0.0,
             'neg': float((allpre[vp] < 0).float().mean()) if nv else 0.0,
             'dmel_nonzero': float((grad0[v3.expand_as(grad0)] != 0).float().mean()) if nv else 0.0}
    return {'pp': pp0, 'pre': pre0, 'signs': sg0, 'grad': grad0, 'dmel': dmel, 'stats': stats}


def mask_check_region(l, lens, T, rows_exist, device):
    """(B, T) bool: the frames on which layer l's sign words are defined by the contract: n < lens[b], and past the length the frames
    the backward reads, n <= lens[b] + 2 - l, where they exist; none for an utterance of length zero (no tile runs)."""
    lens_t = torch.as_tensor(lens, device=device).long()
    n = torch.arange(T, device=device)[None, :]
    m = (n <= lens_t[:, None] + 2 - l) & (lens_t[:, None] > 0)
    return m & exist_mask(len(lens), T, rows_exist, device)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the dense random network (rounded tier)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gauss(g, shape):
    """Near-normal deviates (mean 0, variance 1, |x| < 4.25) built from integer draws alone: the sum of six uniform 16-bit integers,
    scaled by one correctly rounded multiplication.  torch.randn goes through vectorised log / sin / cos, and a last-bit difference
    between two machines there (or in a reduction such as a norm) re-draws every rare rounding flip downstream: the floors below are
    maxima over such flips and would not reproduce.  Integer draws and correctly rounded element-wise arithmetic do."""
    s = torch.randint(-2 ** 15, 2 ** 15, (6,) + tuple(shape), generator=g).sum(0)
    return s.float() * (2.0 ** -15 * 0.7071067811865476)      # variance of the sum: 6 * (2^16)^2 / 12 = 2^31, its root 2^15.5


def dense_state(seed=7, n_mel=80):
    """A seeded PitchPredictor state dict whose folded weights are the same bits on every machine: weight_v = 0.3 x deviates, weight_g
    = ||v|| x 2^-k with the norm as ``fold_pitch_predictor`` computes it, so that g / ||v|| is exactly 2^-k and the folded weight is v
    scaled by a power of two (row norms near 0.5 and near 1); BatchNorm weights ~ N(0, 1) (scales of both signs), running variances
    4^k - eps for k in {-1, 0, 1} (sqrt(var + eps) is exactly 2^k: a vectorised sqrt was seen to differ by an ulp between two machines on
    other values), everything else 0.2 x deviates."""
    import math
    from ubisoft_laforge_daft_exprt_amd import loss as L
    g = torch.Generator().manual_seed(seed)
    shapes = L.pitch_predictor_shapes(n_mel)
    state = {}
    for k, shape in shapes.items():
        if k.endswith('num_batches_tracked'):
            state[k] = torch.tensor(10)
        elif k.endswith('running_var'):
            q = torch.tensor([0.25, 1.0, 4.0])[torch.randint(0, 3, shape, generator=g)]
            state[k] = q - 1e-5                  # var + eps rounds back to a power of 4: its root and the division by it are exact
            assert torch.equal(torch.sqrt(state[k] + 1e-5), torch.sqrt(q)) and torch.equal(torch.sqrt(q) ** 2, q)
        elif k.endswith('weight_g'):
            continue
        elif '.conv.' not in k and k.endswith('.weight'):
            state[k] = _gauss(g, shape)
        else:
            state[k] = _gauss(g, shape) * (0.3 if 'weight_v' in k else 0.2)
    for k, shape in shapes.items():
        if k.endswith('weight_g'):
            v = state[k[:-1] + 'v'].float()
            k0 = math.floor(math.log2(0.3 * math.sqrt(v.shape[1] * v.shape[2])))
            c = torch.where(torch.randint(0, 2, shape, generator=g) == 0, 2.0 ** -k0, 2.0 ** -(k0 + 1))       # (no tensor pow: exact powers)
            state[k] = v.norm(dim=(1, 2), keepdim=True) * c
    return state


ROUNDED_CASES = {
    'lengths': (80, 300, [1, 122, 123, 243, 300, 57]),
    'many': (80, 9, EXACT_CASES['many'][2]),
}
MANY_ALONE = (0, 63, 64, 65, 255, 256, 257, 319)     # rows of 'many' that must equal the same rows launched alone


def rounded_inputs(name, device='cpu'):
    """(mel, dpp, base, lens) of a rounded-tier case: log-mel-like values on every stored frame (past the lengths too), dpp = normal
    deviates masked to the lengths, a nonzero base of the gradient's magnitude (its fp32 addition is part of the floor's orders)"""
    M, T, lens = ROUNDED_CASES[name]
    B = len(lens)
    g = torch.Generator().manual_seed(3000 + len(name))
    mel = (_gauss(g, (B, M, T)) * 1.5 - 5).clamp(-11.5, 2)
    dpp = _gauss(g, (B, T)) * valid_mask(lens, T, 'cpu')
    base = _gauss(g, (B, M, T)) * 0.125
    return mel.to(device), dpp.to(device), base.to(device), lens


def err_figures(dev, ref, region):
    """(max, mean) of |dev - ref| over the bool region"""
    e = (dev.double() - ref).abs()[region]
    return (float(e.max()), float(e.mean())) if e.numel() else (0.0, 0.0)


def rounded_reference(layers, mel, dpp, base, lens, mode):
    """float64 results of a rounded-tier case and their spread over the fp32 summation orders.  Returns pp, pre, signs, grad (linearised
    at float64's own signs), floor {pp_max, pp_mean, dmel_max, dmel_mean}, and per layer the largest |v64| at which an order disagrees with
    float64 in sign (``flip``) and the largest |v32 - v64| (``dist``), for ``mask_tau``."""
    B, M, T = mel.shape
    v = valid_mask(lens, T, mel.device)
    v3 = v[:, None, :].expand(B, M, T)
    pp, pre = chain64(mel, layers, mode, lens)
    sg = signs64(pre)
    grad = chain64_bwd(dpp, sg, layers, mode)
    want = add_base(base, grad, lens)
    floor = {'pp_max': 0.0, 'pp_mean': 0.0, 'dmel_max': 0.0, 'dmel_mean': 0.0}
    flip = [0.0, 0.0, 0.0]
    dist = [0.0, 0.0, 0.0]
    for order in ORDERS:
        pp_o, pre_o = chain64(mel, layers, mode, lens, order=order)
        mx, mn = err_figures(pp_o, pp, v)
        floor['pp_max'], floor['pp_mean'] = max(floor['pp_max'], mx), max(floor['pp_mean'], mn)
        got = add_base(base, chain64_bwd(dpp, sg, layers, mode, order=order), lens, order)
        mx, mn = err_figures(got, want, v3)
        floor['dmel_max'], floor['dmel_mean'] = max(floor['dmel_max'], mx), max(floor['dmel_mean'], mn)
        for l in range(3):
            region = mask_check_region(l, lens, T, None, mel.device)[:, None, :].expand_as(pre[l])
            a, b = pre[l][region], pre_o[l][region]
            dis = (a > 0) != (b > 0)
            if bool(dis.any()):
                flip[l] = max(flip[l], float(a[dis].abs().max()))
            dist[l] = max(dist[l], float((a - b).abs().max()))
    return {'pp': pp, 'pre': pre, 'signs': sg, 'grad': grad, 'floor': floor, 'flip': flip, 'dist': dist, 'lens': lens}


def mask_tau(refs):
    """tau[l] of a mode from the ``rounded_reference`` results of all its cases (like the floors: one figure per mode, the largest over
    the orders and the cases): 4 x the largest |v64| at which an fp32 order disagrees with float64 in sign; where none ever does
    (layer 0, whose input no order can change), 4 x the largest |v32 - v64|."""
    tau = []
    for l in range(3):
        flip, dist = max(r['flip'][l] for r in refs), max(r['dist'][l] for r in refs)
        tau.append(BAR_FACTOR * (flip if flip > 0 else dist))
    return tau


def mask_clear(ref, tau, l, rows_exist=None):
    """(region, clear) of layer l, both (B, 256, T) bool: the contracted sign bits, and those of them with |v64| > tau[l]"""
    v = ref['pre'][l]
    region = mask_check_region(l, ref['lens'], v.shape[2], rows_exist, v.device)[:, None, :].expand_as(v)
    return region, region & (v.abs() > tau[l])


def mask_excluded(ref, tau):
    """share of the contracted sign bits of a case that sit within tau of zero"""
    near = tot = 0
    for l in range(3):
        region, clear = mask_clear(ref, tau, l)
        near += int(region.sum()) - int(clear.sum())
        tot += int(region.sum())
    return near / max(tot, 1)


def dense_layers(device='cpu', rt=None):
    from ubisoft_laforge_daft_exprt_amd import loss as L
    return L.fold_pitch_predictor(dense_state(), device, rt)


def measure_floor(mode):
    """the four floor figures of ``mode``: the largest over the rounded tier's cases (and, inside, over ``ORDERS``)"""
    layers = dense_layers()
    out = {'pp_max': 0.0, 'pp_mean': 0.0, 'dmel_max': 0.0, 'dmel_mean': 0.0}
    for name in ROUNDED_CASES:
        mel, dpp, base, lens = rounded_inputs(name)
        f = rounded_reference(layers, mel, dpp, base, lens, mode)['floor']
        out = {k: max(out[k], f[k]) for k in out}
    return out
