"""The attention tier without a GPU (tests/attn_exact_helpers.py): the hard-attention construction is exact in fp32, every designed input has
the property its name states, the plain-torch emulations pass every element-wise bound, and each planted fault breaks one."""
import math

import pytest
import torch

from tests import attn_exact_helpers as ax
from tests import helpers
from tests.test_attention_dropout import BARS

S1, S2, S4 = ax.SHAPES['S1'], ax.SHAPES['S2'], ax.SHAPES['S4']
HARD = dict(N=256, lens=[256, 192, 128])
SEED = 0xABCDEF1234


def host_keep(B, heads, N, lens, p):
    return helpers.host_attention_keep(SEED, B, heads, N, p) & helpers.attention_valid(lens, heads, N)


def scores64(qkv, heads):
    B, N, D3 = qkv.shape
    q, k = (t.double().reshape(B, N, heads, 64).transpose(1, 2) for t in qkv.split(D3 // 3, dim=2)[:2])
    return (q @ k.transpose(-1, -2)) * 0.125


def test_hard_attention_is_exact_in_fp32():
    """fp32 torch equals float64 to below 1e-50 on ctx, dq, dk, dv, all of them non-zero; lse is 128 + log 2 for classes of two and exactly
    128 for classes of one, whose dq and dk are exactly zero and whose dv is the sum of the dO rows that attend to the key (its own)."""
    N, lens = HARD['N'], HARD['lens']
    qkv, dctx = ax.hard_inputs(N, lens)
    ref = helpers.attention_reference64(qkv, dctx, lens, 2)
    emu = helpers.attention_emulation(qkv, lens, 2, dctx=dctx)
    for name, a, r in zip(('ctx', 'dq', 'dk', 'dv'), emu, (ref[0],) + tuple(ref[2:])):
        assert a.dtype == torch.float32 and float((a.double() - r).abs().max()) < 1e-50, name
        assert float(a[0].abs().max()) > 0, name
    # the tiled emulation recomputes P from a ROUNDED lse, as the kernels do: only its forward is exact for classes of two
    assert float((ax.tiled_emulation(qkv, dctx, lens, 2)['ctx'].double() - ref[0]).abs().max()) < 1e-50
    size = ax.class_size(N, lens)
    assert sorted(size.unique().tolist()) == [0, 1, 2]
    s = scores64(qkv, 2)
    eye = (torch.arange(N)[:, None] - torch.arange(N)[None, :]) % 128 == 0
    assert bool((s[:, :, eye] == 128).all()) and float(s[:, :, ~eye].max()) <= 4.0
    t = ax.tiled_emulation(qkv, dctx, lens, 2)
    one, two = (size == 1), (size == 2)
    lse = t['lse'].transpose(1, 2)                                               # (B, N, H)
    assert bool((lse[one] == 128.0).all()) and bool((lse[two] == torch.tensor(128 + math.log(2.0)).float()).all())
    assert not t['dq'][one].any() and not t['dk'][one].any() and torch.equal(t['dv'][one], dctx[one])
    assert float((ref[1].transpose(1, 2)[two] - (128 + math.log(2.0))).abs().max()) < 1e-12


@pytest.mark.parametrize('rounding', ['f32', 'bf16', 'fp16'])
@pytest.mark.parametrize('kind', ax.KINDS)
def test_each_kind_of_input_has_the_property_its_name_states(kind, rounding):
    """from float64 scores of the (rounded) operands at S1: which key tile holds each query's maximum, by how much it rises from tile to
    tile, and how many queries of a wave of 16 see a new maximum in a later tile"""
    N, lens, heads = S1['N'], S1['lens'], 2
    qkv, _ = ax.make_inputs(kind, N, lens, heads)
    qkv = ax.round_inputs(rounding, qkv)
    s = scores64(qkv, heads)
    for b, n in enumerate(lens):
        sv = s[b, :, :n, :n]                                                     # (H, q, key)
        tiles = [sv[:, :, 64 * t:min(64 * t + 64, n)].amax(-1) for t in range((n + 63) // 64)]
        run = [tiles[0]]
        for t in tiles[1:]:
            run.append(torch.maximum(run[-1], t))
        raised = [tiles[t] > run[t - 1] for t in range(1, len(tiles))]          # (H, q) per later tile
        pmax = torch.softmax(sv, -1).amax(-1)
        if kind == 'randn':
            assert float(pmax.max()) < 0.5 and float(sv.abs().max()) < 8
        elif kind == 'peaked':
            assert float(sv.max()) > 25 and float(sv.min()) < -25 and float(pmax.max()) > 0.9
        elif kind == 'rising':
            assert all(float((tiles[t] - tiles[t - 1]).min()) >= 6.0 for t in range(1, len(tiles)))
            assert all(bool(r.all()) for r in raised)
        elif kind == 'first':
            assert bool((sv.argmax(-1) == 0).all()) and float((sv[:, :, 0] - sv[:, :, 1:].amax(-1)).min()) >= 20 if n > 1 else True
            assert not any(bool(r.any()) for r in raised)
        elif kind == 'last':
            assert bool((sv.argmax(-1) == n - 1).all())
            if n < N:
                assert float((s[b, :, :n, n] - sv.amax(-1)).min()) >= 20           # the padded key would win by far
        elif kind == 'one lane':
            for r in raised:
                per_wave = r[:, :16 * (n // 16)].reshape(heads, -1, 16)
                assert bool((per_wave.sum(-1) == 1).all()) and bool(per_wave[:, :, ax.LANE].all())
                assert int(r[:, 16 * (n // 16):].sum()) == int(n % 16 > ax.LANE) * heads
        elif kind == 'negative':
            assert float(sv.max()) <= -30
        elif kind == 'underflow':
            if len(tiles) == 3:
                assert float((tiles[2] - tiles[0]).min()) >= 190 and float((tiles[1] - tiles[0]).min()) >= 90


def emulate_and_check(mode, kind, shape, p, emulation, heads=2):
    N, lens = shape['N'], shape['lens']
    B = len(lens)
    qkv, dctx = ax.round_inputs(mode, *ax.make_inputs(kind, N, lens, heads))
    keep = host_keep(B, heads, N, lens, p) if p else None
    h16 = ax.H16.get(mode)
    bad, figs = [], []
    for name, qdt, cdt, odt in ax.variants(mode):
        bd = ax.bounds(qkv, dctx, lens, heads, mode, keep, p, ctx_store=mode if cdt != torch.float32 else None)
        if emulation == 'helpers':
            ctx, dq, dk, dv = helpers.attention_emulation(qkv, lens, heads, keep, p, h16, dctx)
            got = dict(ctx=ctx, dq=dq, dk=dk, dv=dv)
        else:
            got = ax.tiled_emulation(qkv, dctx, lens, heads, keep, p, h16)
        got['ctx'] = got['ctx'].to(cdt)
        for n in ('dq', 'dk', 'dv'):
            got[n] = got[n].to(odt)
        stores = dict(ctx=cdt, dq=odt, dk=odt, dv=odt)
        b, r = ax.check_all(got, bd, lens, stores, tag=f'{mode} {kind} p={p} ({name})')
        bad += b
        figs.append(r)
    return bad, figs


@pytest.mark.parametrize('emulation', ['helpers', 'tiled'])
@pytest.mark.parametrize('mode', ax.MODES)
@pytest.mark.parametrize('kind', ax.KINDS)
def test_the_emulations_pass_every_bound(kind, mode, emulation):
    """helpers.attention_emulation and the tiled emulation, in fp32 and with the 16-bit roundings, every storage variant, p = 0 and p = 0.1,
    S1 and S2 (S4 for 'last'): every element of every output inside its bound, padded rows exactly zero"""
    bad = []
    for shape in (S1, S2) + ((S4,) if kind == 'last' else ()):
        for p in (0.0, 0.1):
            b, figs = emulate_and_check(mode, kind, shape, p, emulation)
            print(f'{emulation} {mode} {kind} N={shape["N"]} p={p}: ' + ' '.join(f'{n}={max(f.get(n, 0) for f in figs):.2e}' for n in ax.NAMES))
            bad += b
    assert not bad, bad


def test_the_tiled_emulation_applies_the_mask_it_is_given():
    """helpers.recover_keep reads the host mask back out of the tiled emulation's forward: its dropout sits where the kernels' does"""
    N, lens, heads, p = S1['N'], S1['lens'], 2, 0.1
    keep = host_keep(len(lens), heads, N, lens, p)
    zeros = torch.zeros(len(lens), N, 64 * heads)
    fwd = lambda x: ax.tiled_emulation(x, zeros, lens, heads, keep, p)['ctx']
    assert torch.equal(helpers.recover_keep(fwd, len(lens), N, heads, lens, p), keep)


FAULT_CASES = {'stale alpha': ('rising', 0.0), 'tail + 1': ('last', 0.0), 'tail - 1': ('last', 0.0), 'lse after dropout': ('randn', 0.1),
               'no QSCALE in dK': ('randn', 0.0), 'delta of the other head': ('randn', 0.0), 'pairs swapped': ('randn', 0.0)}


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('fault', ax.FAULTS)
def test_every_planted_fault_breaks_a_bound(fault, mode):
    """Each fault, planted in the tiled emulation on the kind of input designed for it, leaves some element outside its bound (printed:
    by how much) and changes bits against the sound emulation.  For the stale alpha and the off-by-one tail masks also printed: what the
    whole-component norm ratio on randn inputs shows for the same fault, next to its bar."""
    kind, p = FAULT_CASES[fault]
    N, lens, heads = S1['N'], S1['lens'], 2
    qkv, dctx = ax.round_inputs(mode, *ax.make_inputs(kind, N, lens, heads))
    keep = host_keep(len(lens), heads, N, lens, p) if p else None
    h16 = ax.H16.get(mode)
    bd = ax.bounds(qkv, dctx, lens, heads, mode, keep, p)
    sound = ax.tiled_emulation(qkv, dctx, lens, heads, keep, p, h16)
    wrong = ax.tiled_emulation(qkv, dctx, lens, heads, keep, p, h16, fault=fault)
    assert not ax.check_all(sound, bd, lens, {})[0]
    bad, ratios = ax.check_all(wrong, bd, lens, {})
    print(f'[{mode}] {fault} on {kind}: measured / bound ' + ' '.join(f'{n}={ratios[n]:.3g}' for n in ax.NAMES))
    assert bad and max(ratios.values()) > 1.0, ratios
    assert any(not torch.equal(sound[n], wrong[n]) for n in ax.NAMES)
    if fault in ('stale alpha', 'tail + 1', 'tail - 1'):
        rq, rd = ax.round_inputs(mode, *ax.make_inputs('randn', N, lens, heads))
        rb = ax.bounds(rq, rd, lens, heads, mode)
        rw = ax.tiled_emulation(rq, rd, lens, heads, None, 0.0, h16, fault=fault)
        norm = ax.bars_ratio(rw, rb['ref'])
        elem = ax.check_all(rw, rb, lens, {})[1]
        print(f'[{mode}] {fault} on randn: norm ratio ' + ' '.join(f'{n}={norm[n]:.2e}' for n in norm) + f' (bars {BARS[mode]});'
              f' measured / bound ' + ' '.join(f'{n}={elem[n]:.3g}' for n in ax.NAMES))
