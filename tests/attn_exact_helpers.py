"""The attention kernels of csrc/dx_attention.hip restated: designed inputs, a float64 reference with element-wise a-priori bounds, a tiled
fp32 emulation of the online softmax that can carry planted faults, and the shapes of tests/test_attn_exact_cpu.py and
tests/test_attn_exact_gpu.py.

Everything is per (utterance, head): s = q k^T / 8 on valid keys, P = softmax(s), ctx = (P keep / (1 - p)) v, lse = logsumexp(s),
dv = (P keep / (1 - p))^T g, dP = g v^T, delta = g . ctx, dS = P (dP keep / (1 - p) - delta), dq = dS k / 8, dk = dS^T q / 8.
In the 16-bit modes the inputs are rounded to the 16-bit type first, so the float64 reference sees the operands the kernels see.

Bounds (``bounds``; u = 2^-24, u_h the 16-bit unit roundoff, sub = 2^-25 half a subnormal step of fp16, all magnitudes float64 of the case
itself, fixed before any device run).  Kernel lines are those of csrc/dx_attention.hip.

  score          d[q, k] = (66 u + u_s) A + 2 (T + 1) u (|s| + max_k |s|) + 4 u |lse| + 4 (T + 1) u + sub ln2 (sum_i |q_i| + sum_i |k_i|)
                 A = sum_i |q_i k_i| / 8 is the 64-term chain (:136 mma4, :892 two K = 32 MFMAs, :498 split3), 66 = 64 + the scale
                 and one conversion; u_s is the operand rounding: 0 in f32, 3 * 2^-16 per split-bf16 product (dx_common.h: hi and lo
                 rounded to nearest leave 2^-16 |x| each, and lo * lo is dropped), u_h + u for q * QSCALE2 (:862, :1129) or k * QSCALE2
                 (:1240) rounded to 16 bits, with sub per element where fp16 reaches its subnormals.  T = key tiles: the exponent of a
                 weight is rounded once per subtraction s - m_new (:156, :915) and once per alpha = exp(m_run - m_new) (:148, :926) it later
                 meets, each on numbers no larger than |s| + max |s|; 4 u per exp (expf 2 ulp, v_exp_f32 1 ulp); in the backward the
                 subtraction is s - lse (:281, :380) or the accumulator that starts at -lse (:1171, :1289).
  amplification  a weight with score error d is off by the factor e^d; the normaliser by at most e^D, D[q] = log sum_k P e^d (Jensen gives
                 the same D for the lower side); the l_run chain (:163, :933) adds (N + 4 T + 8) u =: c.  Forward probabilities:
                 rho_f = expm1(d + D + c).  lse (:187, :975): L = D + c + 4 u (max |s| + |lse| + 1).  Backward probabilities
                 exp(s - lse): rho_b = expm1(d + L): the lse rounding u |lse| is inside L.  A weight below 2^-126 may be flushed: + 2^-120.
  ctx            sum_k Pk |v| ((1 + rho_f)(1 + u_p + c) - 1) + sub / (1 - p) sum_k keep |v|      Pk = P keep / (1 - p); u_p the rounding of
                 the P operand (:935 pack_pair: u_h; split: 3 * 2^-16; f32: 0); c the P V chain and the rescales of o (:169, :931).
  dv             sum_q |g| Pk ((1 + rho_b)(1 + u_p + c) - 1) + sub ...                            (:396, :1325; 1 / (1 - p) rides on dV :1335)
  dP             (66 u + u_g) sum_i |g_i v_i| / (1 - p) + sub (sum |g| + sum |v|)                  u_g: dO / (1 - p) (:1136) or v / (1 - p)
                 (:1241) rounded to 16 bits when p > 0; split: 3 * 2^-16
  delta          sum_d |g_d| E_ctx[d] + 66 u sum_d |g_d ctx_d|, and for a 16-bit-stored context u_h sum |g| (|ctx| + E_ctx) + sub sum |g|
                 (:200, :1138: delta is taken from the STORED context)
  dS             P ((1 + rho_b) E_u + rho_b |u|) + tiny, u = dP keep / (1 - p) - delta, E_u = E_dP + E_delta + 2 u (|dP| / (1 - p) + |delta|);
                 then the dS operand rounding u_p (|dS| + E) + sub (:1193, :1322)
  dq, dk         (E_dS |k|) / 8 + c (|dS| |k|) / 8 over keys (:293, :1197), the same with |q| over queries (:397, :1326)
  16-bit-stored ctx / dqkv: the stored number lies between the 16-bit roundings of (reference - bound) and (reference + bound).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
U_H = {'bf16': 2.0 ** -8, 'fp16': 2.0 ** -11}
SUB_H = {'bf16': 0.0, 'fp16': 2.0 ** -25}
H16 = {'bf16': torch.bfloat16, 'fp16': torch.float16}
UX3 = 3.0 * 2.0 ** -16
TINY = 2.0 ** -120
LN2 = math.log(2.0)
MODES = ('f32', 'bf16x3', 'bf16', 'fp16')
NAMES = ('ctx', 'lse', 'dq', 'dk', 'dv')
QSCALE2 = float(np.float32(0.125) * np.float32(1.4426950408889634))       # csrc/dx_attention.hip QSCALE2, an fp32 product

SHAPES = {
    'S1': dict(N=192, lens=[192, 130, 65]),                 # three key tiles, ragged tails
    'S2': dict(N=37, lens=[37, 5, 1]),                      # N < 64
    'S3': dict(N=130, lens=[130, 0, 64]),                   # a zero-length utterance
    'S4': dict(N=130, lens=[130, 129, 64, 1]),              # B x H = 8: the renumbered workgroups
}
S4_LENS8 = [130, 129, 64, 1, 100, 65, 2, 128]             # S4 with 8 utterances, for H = 1 and H = 4
KINDS = ('randn', 'peaked', 'rising', 'first', 'last', 'one lane', 'negative', 'underflow')
LANE = 5                                                    # the query of each wave of 16 that 'one lane' lets rise


def variants(mode):
    from tests.test_attention_dropout import variants as v
    return v(mode)


def round_inputs(mode, *ts):
    """the 16-bit modes round every input to the 16-bit type before anything else (returned as fp32 holding those values)"""
    if mode not in H16:
        return ts if len(ts) > 1 else ts[0]
    out = tuple(t.to(H16[mode]).float() for t in ts)
    return out if len(out) > 1 else out[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def make_inputs(kind, N, lens, heads=2, seed=0):
    """(qkv (B, N, 3 D), dctx (B, N, D)), fp32 on the CPU, dctx zero on padded queries.  Channel 0 of every head is a key bias (q = 8 there,
    so the score gains k[key, 0]), channel 1 a query-times-key term (q = 8 x[query], so the score gains x[query] k[key, 1]); the other 62
    channels are 0.5 randn (score noise of standard deviation 0.25).  Every planted number is exact in bf16."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 7 * N + heads + seed)
    B, D = len(lens), 64 * heads
    qkv = torch.randn(B, N, 3 * D, generator=g)
    dctx = torch.randn(B, N, D, generator=g)
    inside = torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    dctx = dctx * inside[:, :, None]
    if kind == 'randn':
        return qkv, dctx
    if kind == 'peaked':
        qkv[:, :, :2 * D] *= 3.0
        return qkv, dctx
    qkv[:, :, :2 * D] *= 0.5
    idx = torch.arange(N)
    tile = (idx // 64).float()
    for h in range(heads):
        q0, q1, k0, k1 = 64 * h, 64 * h + 1, D + 64 * h, D + 64 * h + 1
        qkv[:, :, q0], qkv[:, :, q1], qkv[:, :, k0], qkv[:, :, k1] = 8.0, 0.0, 0.0, 0.0
        if kind == 'rising':
            qkv[:, :, k0] = 9.0 * tile
        elif kind == 'first':
            qkv[:, 0, k0] = 30.0
        elif kind == 'last':
            for b, n in enumerate(lens):
                if n >= 1:
                    qkv[b, n - 1, k0] = 30.0
                if n < N:
                    qkv[b, n, k0] = 60.0              # the first padded row: an even larger would-be score
        elif kind == 'one lane':
            qkv[:, 0, k0] = 6.0
            qkv[:, :, q1] = 8.0 * (idx % 16 == LANE).float()
            qkv[:, :, k1] = 10.0 * tile
        elif kind == 'negative':
            qkv[:, :, k0] = -40.0
        elif kind == 'underflow':
            qkv[:, :, k0] = 100.0 * tile
    return qkv, dctx


def hard_inputs(N, lens, heads=2, seed=0):
    """Hard attention: token i = 64 t + a has q = sigma_t 32 e_a, sigma = +1 in even key tiles and -1 in odd ones, and k = the same vector
    plus multiples of 1/4 in [-1, 1] off its own axis; v and dctx are multiples of 1/4 in [-2, 2].  Score 128 between tokens of one axis and
    one sign (i and i +- 128), -128 for the other sign, at most 4 in magnitude elsewhere: every softmax is exactly 0 / 1/2 / 1 in fp32."""
    g = torch.Generator().manual_seed(4242 + N + heads + seed)
    B, D = len(lens), 64 * heads
    idx = torch.arange(N)
    sign = 1.0 - 2.0 * ((idx // 64) % 2).float()
    axis = torch.nn.functional.one_hot(idx % 64, 64).float()                      # (N, 64)
    dy = lambda *shape, m: torch.randint(-m, m + 1, shape, generator=g).float() / 4
    qkv = torch.zeros(B, N, 3 * D)
    for h in range(heads):
        qkv[:, :, 64 * h:64 * h + 64] = 32.0 * sign[:, None] * axis
        qkv[:, :, D + 64 * h:D + 64 * h + 64] = 32.0 * sign[:, None] * axis + dy(B, N, 64, m=4) * (1 - axis)
    qkv[:, :, 2 * D:] = dy(B, N, D, m=8)
    inside = torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    dctx = dy(B, N, D, m=8) * inside[:, :, None]
    return qkv, dctx


def class_size(N, lens):
    """(B, N): how many valid keys share token i's axis and sign (0 on padded rows)"""
    idx = torch.arange(N)
    same = ((idx[:, None] - idx[None, :]) % 128 == 0)
    inside = idx[None, :] < torch.tensor(lens)[:, None]
    return (same[None] & inside[:, None, :]).sum(-1) * inside


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ------------------------------------------------------------------------------------------------------------------------------------
def _split(t, B, N, heads):
    return t.reshape(B, N, heads, 64).transpose(1, 2)


def _merge(t):
    B, H, N, _ = t.shape
    return t.transpose(1, 2).reshape(B, N, H * 64)


def bounds(qkv, dctx, lens, heads, mode, keep=None, p=0.0, ctx_store=None):
    """float64 reference and element-wise bound of ctx, lse (natural log), dq, dk, dv for operand mode ``mode`` on the (already rounded)
    operands ``qkv`` / ``dctx``; ``ctx_store``: the 16-bit mode name when the context handed to the backward is 16-bit stored.  Returns
    {'ref': {...}, 'bnd': {...}, 'P': probabilities (B, H, N, N), 'EPf' / 'EPb': bounds on the forward's / backward's probabilities}."""
    qkv, dctx = qkv.detach().cpu().double(), dctx.detach().cpu().double()
    B, N, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (_split(t, B, N, heads) for t in qkv.split(D, dim=2))
    lens_t = torch.as_tensor(lens, dtype=torch.long).cpu()
    inside = torch.arange(N)[None, :] < lens_t[:, None]
    kv, qv = inside[:, None, None, :], inside[:, None, :, None].double()
    g = _split(dctx, B, N, heads) * qv
    T = (int(lens_t.max()) + 63) // 64
    h16 = mode in H16
    u_s = {'f32': 0.0, 'bf16x3': UX3}.get(mode, U_H.get(mode, 0.0) + U)
    u_p = {'f32': 0.0, 'bf16x3': UX3}.get(mode, U_H.get(mode, 0.0))
    drop = keep is not None and p > 0
    u_g = {'f32': 0.0, 'bf16x3': UX3}.get(mode, U_H.get(mode, 0.0) if drop else 0.0)
    sub = SUB_H.get(mode, 0.0)
    sc = 1.0 / (1.0 - p) if drop else 1.0
    km = keep.detach().cpu().double() if drop else torch.ones(B, heads, N, N, dtype=torch.float64)
    km = km * kv

    s = (q @ k.transpose(-1, -2)) * 0.125
    A = (q.abs() @ k.abs().transpose(-1, -2)) * 0.125
    sabs = (s.abs() * kv).amax(-1, keepdim=True)
    sm = s.masked_fill(~kv, float('-inf'))
    some = inside.any(1)[:, None, None, None]
    lse = torch.where(some, torch.logsumexp(sm, dim=-1, keepdim=True), torch.zeros(()).double())
    P = torch.where(some, torch.exp(sm - lse), torch.zeros(()).double())
    d = ((66 * U + u_s) * A + 2 * (T + 1) * U * (s.abs() + sabs) + 4 * U * lse.abs() + 4 * (T + 1) * U
         + sub * LN2 * (q.abs().sum(-1, keepdim=True) + k.abs().sum(-1)[:, :, None, :]))
    c = (N + 4 * T + 8) * U
    Dq = torch.log((P * torch.exp(d)).sum(-1, keepdim=True).clamp_min(1.0))
    rho_f = torch.expm1(d + Dq + c)
    L = Dq + c + 4 * U * (sabs + lse.abs() + 1)
    rho_b = torch.expm1(d + L)
    EPf = (P * rho_f + TINY) * kv
    EPb = (P * rho_b + TINY) * kv * qv

    Pk = P * km * sc
    ctx = (Pk @ v) * qv
    op = lambda rho: (1 + rho) * (1 + u_p + c) - 1
    Ectx = (((Pk * op(rho_f) + TINY) @ v.abs()) + sub * sc * (km @ v.abs())) * qv
    Pq = Pk * qv
    dv = Pq.transpose(-1, -2) @ g
    Edv = ((Pq * op(rho_b) + TINY * km * qv).transpose(-1, -2) @ g.abs()) + sub * sc * ((km * qv).transpose(-1, -2) @ g.abs())

    dP = g @ v.transpose(-1, -2)
    EdP = ((66 * U + u_g) * (g.abs() @ v.abs().transpose(-1, -2)) + sub * (g.abs().sum(-1, keepdim=True) + v.abs().sum(-1)[:, :, None, :])) * sc
    delta = (g * ctx).sum(-1, keepdim=True)
    Edelta = (g.abs() * Ectx).sum(-1, keepdim=True) + 66 * U * (g * ctx).abs().sum(-1, keepdim=True)
    if ctx_store is not None:
        Edelta = Edelta + U_H[ctx_store] * (g.abs() * (ctx.abs() + Ectx)).sum(-1, keepdim=True) + SUB_H[ctx_store] * g.abs().sum(-1, keepdim=True)
    u = dP * km * sc - delta
    Eu = EdP * km + Edelta + 2 * U * (dP.abs() * sc + delta.abs())
    Pv = P * kv * qv
    dS = Pv * u
    EdS = Pv * ((1 + rho_b) * Eu + rho_b * u.abs()) + TINY * (u.abs() + Eu) * kv * qv
    EdS = EdS + u_p * (dS.abs() + EdS) + sub * kv * qv
    dq = (dS @ k) * 0.125
    Edq = (EdS @ k.abs()) * 0.125 + c * (dS.abs() @ k.abs()) * 0.125
    dk = (dS.transpose(-1, -2) @ q) * 0.125
    Edk = (EdS.transpose(-1, -2) @ q.abs()) * 0.125 + c * (dS.abs().transpose(-1, -2) @ q.abs()) * 0.125

    sq = lambda t: (t * qv).squeeze(-1)
    ref = dict(ctx=_merge(ctx), lse=sq(lse), dq=_merge(dq), dk=_merge(dk), dv=_merge(dv))
    bnd = dict(ctx=_merge(Ectx), lse=sq(L), dq=_merge(Edq), dk=_merge(Edk), dv=_merge(Edv))
    return dict(ref=ref, bnd=bnd, P=P * kv * qv, EPf=EPf * qv, EPb=EPb)


def between(got, ref, bnd, store=None):
    """bool tensor, True where ``got`` misses: |got - ref| <= bnd for an fp32 result (one more u |ref| for the last fp32 rounding); for a result
    stored in 16 bits (``store``: torch dtype) it must lie between the 16-bit roundings of the fp32 bound's ends"""
    got = got.detach().cpu()
    bnd = bnd + U * ref.abs()
    if store in (None, torch.float32):
        return ~((got.double() - ref).abs() <= bnd)
    lo, hi = (ref - bnd).float().to(store).double(), (ref + bnd).float().to(store).double()
    return ~((got.double() >= lo) & (got.double() <= hi))


def ratio(got, ref, bnd, store=None):
    """largest |got - ref| / bound over all elements (for a 16-bit-stored result the bound gains that rounding); 0 / 0 counts as 0"""
    got = got.detach().cpu().double()
    bnd = bnd + U * ref.abs()
    if store not in (None, torch.float32):
        m = 'bf16' if store == torch.bfloat16 else 'fp16'
        bnd = bnd + U_H[m] * (ref.abs() + bnd) + SUB_H[m]
    e = (got - ref).abs()
    r = torch.where(e == 0, torch.zeros_like(e), e / bnd.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def padded_rows_zero(lens, **outs):
    """names of the outputs with a non-zero element in a padded row (ctx / dq / dk / dv: (B, N, D); lse: (B, H, N))"""
    bad = []
    for name, t in outs.items():
        for b, n in enumerate(lens):
            rows = t[b, :, n:] if name == 'lse' else t[b, n:]
            if rows.any():
                bad.append((name, b))
    return bad


def check_all(got, bd, lens, stores, tag=''):
    """``got``: dict of device / CPU results (lse in natural log), compared element by element with ``bd = bounds(...)``; ``stores``: storage type
    per name.  Returns (misses, ratios): misses lists (tag, name, count, worst ratio); every element counts, padded rows must be zero."""
    bad, ratios = [], {}
    for name in NAMES:
        if name not in got:
            continue
        t = got[name].detach().cpu()
        miss = between(t, bd['ref'][name], bd['bnd'][name], stores.get(name))
        ratios[name] = ratio(t, bd['ref'][name], bd['bnd'][name], stores.get(name))
        if not bool(torch.isfinite(t.double()).all()):
            bad.append((tag, name, 'not finite'))
        if miss.any():
            bad.append((tag, name, int(miss.sum()), ratios[name], miss.nonzero()[0].tolist()))
    bad += [(tag,) + z + ('padded row not zero',) for z in padded_rows_zero(lens, **{n: got[n].detach().cpu() for n in got if n in NAMES})]
    return bad, ratios


# ------------------------------------------------------------------------------------------------------------------------------------
# the probability read-out
# ------------------------------------------------------------------------------------------------------------------------------------
def readout_forward_passes(qkv, heads):
    """Inputs that read P out of a forward: pass j replaces V by the identity on key block j (helpers.recover_keep's protocol), so the
    context of ``x`` is ctx[b, q, 64 h + c] = P[b, h, q, 64 j + c] (times keep / (1 - p) under dropout).  Yields (j, x)."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    for j in range((N + 63) // 64):
        k0, k1 = 64 * j, min(64 * j + 64, N)
        x = qkv.clone()
        x[:, :, 2 * D:] = 0
        for h in range(heads):
            x[:, k0:k1, 2 * D + 64 * h:2 * D + 64 * h + (k1 - k0)] = torch.eye(k1 - k0)
        yield j, x


def readout_dkv_passes(N, lens, heads):
    """Upstream gradients that read P out of the dK/dV kernel: pass i sends dctx[64 i + c, 64 h + c] = 1 on the valid queries of block i,
    so dv[b, key, 64 h + c] = P[b, h, 64 i + c, key].  Yields (i, dctx)."""
    B, D = len(lens), 64 * heads
    inside = torch.arange(N)[None, :] < torch.tensor(lens)[:, None]
    for i in range((N + 63) // 64):
        q0, q1 = 64 * i, min(64 * i + 64, N)
        dctx = torch.zeros(B, N, D)
        for h in range(heads):
            dctx[:, q0:q1, 64 * h:64 * h + (q1 - q0)] = torch.eye(q1 - q0)
        yield i, dctx * inside[:, :, None]


def probability_figures(got, ref, floor=1e-6):
    """(largest |P_dev - P|, largest |P_dev - P| / P over the elements with P >= floor) of a read-out component"""
    e = (got.detach().cpu().double() - ref).abs()
    big = ref >= floor
    return float(e.max()), float((e[big] / ref[big]).max()) if big.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# a tiled fp32 emulation that can be wrong on purpose
# ------------------------------------------------------------------------------------------------------------------------------------
FAULTS = ('stale alpha', 'tail + 1', 'tail - 1', 'lse after dropout', 'no QSCALE in dK', 'delta of the other head', 'pairs swapped')


def tiled_emulation(qkv, dctx, lens, heads, keep=None, p=0.0, h16=None, fault=None):
    """The kernels' arithmetic in fp32 torch, 64-key tiles with the online softmax (m_run, l_run, alpha) as attn_fwd_kernel / attn_key_loop
    run it, and the backward from the saved lse; with ``h16`` the operands are rounded where the 16-bit kernels round them (q * QSCALE2 in
    the forward and dQ, k * QSCALE2 in dK/dV, P, dS) and the scores are in base 2.  Returns ctx, lse (natural log), dq, dk, dv, fp32.
    ``fault`` plants one of ``FAULTS``."""
    assert fault is None or fault in FAULTS
    B, N, D3 = qkv.shape
    D = D3 // 3
    rd = (lambda t: t.to(h16).float()) if h16 is not None else (lambda t: t)
    q, k, v = (_split(t.float(), B, N, heads) for t in qkv.split(D, dim=2))
    lens_t = torch.as_tensor(lens, dtype=torch.long)
    inside = torch.arange(N)[None, :] < lens_t[:, None]
    shift = {'tail + 1': 1, 'tail - 1': -1}.get(fault, 0)
    kin = (torch.arange(N)[None, :] < (lens_t[:, None] + shift).clamp_min(1))[:, None, None, :]
    qv = inside[:, None, :, None].float()
    drop = keep is not None and p > 0
    sc = 1.0 / (1.0 - p) if drop else 1.0
    km = keep.float() if drop else torch.ones(B, heads, N, N)
    if h16 is None:
        ex, lg, unit = torch.exp, torch.log, 1.0
        sq = (q * 0.125) @ k.transpose(-1, -2)
        sk = sq
    else:
        ex, lg, unit = torch.exp2, torch.log2, LN2
        sq = rd(q * QSCALE2) @ k.transpose(-1, -2)
        sk = q @ rd(k * QSCALE2).transpose(-1, -2)
    neg = torch.tensor(float('-inf'))
    m = torch.full((B, heads, N, 1), float('-inf'))
    l = torch.zeros(B, heads, N, 1)
    l_drop = torch.zeros(B, heads, N, 1)
    o = torch.zeros(B, heads, N, 64)
    stale = (torch.arange(N) % 16 == 3)[None, None, :, None]
    for t in range((N + 63) // 64):
        k0, k1 = 64 * t, min(64 * t + 64, N)
        st = torch.where(kin[..., k0:k1], sq[..., k0:k1], neg)
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))
        safe = torch.where(torch.isinf(m_new), torch.zeros(()), m_new)
        alpha = torch.where(torch.isinf(m), torch.zeros(()), ex(m - safe))
        if fault == 'stale alpha' and t >= 1:
            alpha = torch.where(stale, torch.ones(()), alpha)
        e = ex(st - safe) * kin[..., k0:k1]
        l = l * alpha + e.sum(-1, keepdim=True)
        l_drop = l_drop * alpha + (e * km[..., k0:k1] * sc).sum(-1, keepdim=True)
        o = o * alpha + rd(e * km[..., k0:k1]) @ v[:, :, k0:k1]
        m = m_new
    ctx = o * (sc / l) * qv
    lse = torch.where(qv > 0, m + lg(l_drop if fault == 'lse after dropout' else l), torch.zeros(()))
    g = _split(rd(dctx.float()), B, N, heads) * qv
    live = kin & inside[:, None, :, None]
    pq = ex(torch.where(live, sq - lse, neg))
    pk = ex(torch.where(live, sk - lse, neg))
    delta = (g * ctx).sum(-1, keepdim=True)
    if fault == 'delta of the other head':
        delta = delta.flip(1)
    gv = g @ v.transpose(-1, -2)
    if h16 is not None and drop:
        gv = rd(g * sc) @ v.transpose(-1, -2)
    else:
        gv = gv * sc
    u = gv * km - delta
    dq = rd(pq * u) @ k * 0.125
    dk = rd(pk * u).transpose(-1, -2) @ q * (1.0 if fault == 'no QSCALE in dK' else 0.125)
    dv = rd(pk * km).transpose(-1, -2) @ g * sc
    out = [ctx, lse * unit, dq, dk, dv]
    if fault == 'pairs swapped':
        for t in out:
            a, b = t[0, 0].clone(), t[B - 1, heads - 1].clone()
            t[0, 0], t[B - 1, heads - 1] = b, a
    return dict(ctx=_merge(out[0]), lse=out[1].squeeze(-1), dq=_merge(out[2]), dk=_merge(out[3]), dv=_merge(out[4]))


def bars_ratio(got, ref, names=('ctx', 'dq', 'dk', 'dv')):
    """what tests/test_attention_dropout.py measures: max |error| over a whole component / max |reference| over it"""
    return {n: float((got[n].double() - ref[n]).abs().max() / ref[n].abs().max().clamp_min(1e-300)) for n in names}
