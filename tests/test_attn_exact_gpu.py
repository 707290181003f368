"""The attention kernels (csrc/dx_attention.hip: exact f32, split bf16, the templated 16-bit kernels, the fused forward) element by element
against float64 on designed inputs.  Tier 1 is bitwise: the workgroup renumbering is pure scheduling, padded rows do not matter, a
zero-length utterance is zeros and changes nobody else, powers of two pass through, hard attention is exact.  Tier 2 holds every valid
element of ctx, lse, dq, dk and dv to the a-priori bound of tests/attn_exact_helpers.py, and reads the probabilities out of the forward
and out of the dK/dV kernel.  Measured / bound figures are printed and recorded in DESIGN.md."""
import pytest
import torch

from tests import attn_exact_helpers as ax
from tests import helpers
from tests.test_kernels_gpu import _one_launch_vs_two_launches_bitwise

DEV = 'cuda'
SEED = 0xABCDEF1234
HARD = dict(N=256, lens=[256, 192, 128])


@pytest.fixture(scope='module')
def ops():
    from ubisoft_laforge_daft_exprt_amd import ops as _ops
    _ops.set_precision('f32')
    return _ops


class Mode:
    """``with Mode(ops, mode):`` -- the operand mode for the kernel-level calls inside, 'f32' again afterwards"""
    def __init__(self, ops, mode):
        self.ops, self.mode = ops, mode

    def __enter__(self):
        self.ops.set_precision(self.mode)

    def __exit__(self, *exc):
        self.ops.set_precision('f32')


def forward(ops, variant, qkv, lens, heads, p, order=False):
    _, qdt, cdt, _ = variant
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    od = ops.length_order(ln) if order else None
    return ops.attention_fwd(qkv.to(DEV).to(qdt).contiguous(), ln, heads, SEED, p, ctx_dtype=cdt, order=od)


def run(ops, variant, qkv, dctx, lens, heads, p, order=False):
    """ctx, lse (as stored), dqkv of one storage variant, on the CPU"""
    _, qdt, cdt, odt = variant
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
    od = ops.length_order(ln) if order else None
    q = qkv.to(DEV).to(qdt).contiguous()
    ctx, lse = ops.attention_fwd(q, ln, heads, SEED, p, ctx_dtype=cdt, order=od)
    dqkv = ops.attention_bwd(q, ctx, dctx.to(DEV).to(cdt).contiguous(), lse, ln, heads, SEED, p, out_dtype=odt, order=od)
    assert ctx.dtype == cdt and dqkv.dtype == odt and lse.dtype == torch.float32
    return ctx.cpu(), lse.cpu(), dqkv.cpu()


def as_dict(mode, ctx, lse, dqkv):
    """the five components, lse in natural log (the 16-bit kernels save it in base 2)"""
    dq, dk, dv = dqkv.split(dqkv.shape[2] // 3, dim=2)
    return dict(ctx=ctx, lse=lse.double() * (ax.LN2 if mode in ax.H16 else 1.0), dq=dq, dk=dk, dv=dv)


def host_keep(lens, heads, N, p):
    return helpers.host_attention_keep(SEED, len(lens), heads, N, p) & helpers.attention_valid(lens, heads, N)


def same(a, b, n=None):
    return all(torch.equal(x[:n], y[:n]) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 1: bitwise
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('mode', ax.MODES)
@pytest.mark.parametrize('heads,lens', [(2, ax.SHAPES['S4']['lens']), (1, ax.S4_LENS8), (4, ax.S4_LENS8)])
def test_workgroup_renumbering_is_pure_scheduling(ops, heads, lens, mode):
    """heads x utterances divisible by 8 (``xcd_map`` on) against the same utterances with one more appended (off): ctx, lse and dqkv of
    the shared utterances are the same bits, with and without ``order``, at p = 0 and p = 0.1 (the dropout counter depends on
    b * heads + h and N only), fp32 storage and all-16-bit storage."""
    N = ax.SHAPES['S4']['N']
    assert (heads * len(lens)) % 8 == 0 and (heads * (len(lens) + 1)) % 8 != 0
    more = lens + [77]
    qkv, dctx = ax.round_inputs(mode, *ax.make_inputs('randn', N, more, heads))
    B = len(lens)
    bad = []
    with Mode(ops, mode):
        vs = ax.variants(mode)
        for variant in (vs[0], vs[-1]) if len(vs) > 1 else vs:
            for p in (0.0, 0.1):
                base = run(ops, variant, qkv[:B], dctx[:B], lens, heads, p)
                assert all(bool(torch.isfinite(t.double()).all()) for t in base) and float(base[2].abs().max()) > 0
                for order in (False, True):
                    on = base if not order else run(ops, variant, qkv[:B], dctx[:B], lens, heads, p, order=True)
                    off = run(ops, variant, qkv, dctx, more, heads, p, order=order)
                    if not same(on, off, B) or not same(on, base):
                        bad.append((mode, variant[0], p, order))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
@pytest.mark.parametrize('lens_h', [[130, 129, 64, 1, 100, 65, 2, 128], [130, 129, 64, 1, 100, 65, 2, 128, 37, 5, 1, 130, 96, 63, 110, 17]])
def test_fused_forward_is_the_two_launches_at_8_and_16_utterances(ops, precision, lens_h):
    """dx_attention_proj_ln_fwd against dx_attention_fwd + dx_proj_ln_fwd, bit for bit, where the unfused forward renumbers its workgroups"""
    _one_launch_vs_two_launches_bitwise(ops, precision, lens_h, 130, 0.1, 0.1, True)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ax.MODES)
@pytest.mark.parametrize('shape', ['S1', 'S3'])
def test_padded_rows_do_not_matter(ops, shape, mode):
    """rows len .. N of qkv filled with finite values up to +-1e4 (dctx zero there, the contract): every output, every storage variant,
    p = 0 and p = 0.1, is bit for bit what it is with zeros there"""
    N, lens, heads = ax.SHAPES[shape]['N'], ax.SHAPES[shape]['lens'], 2
    qkv, dctx = ax.round_inputs(mode, *ax.make_inputs('randn', N, lens, heads))
    inside = (torch.arange(N)[None, :] < torch.tensor(lens)[:, None])[:, :, None]
    g = torch.Generator().manual_seed(99)
    fill = (torch.rand(qkv.shape, generator=g) * 2 - 1) * 1e4
    fill[:, :, ::7] = 1e4
    fill[:, :, 3::7] = -1e4
    clean = qkv * inside
    dirty = ax.round_inputs(mode, torch.where(inside, qkv, fill))
    bad = []
    with Mode(ops, mode):
        for variant in ax.variants(mode):
            for p in (0.0, 0.1):
                a, b = run(ops, variant, clean, dctx, lens, heads, p), run(ops, variant, dirty, dctx, lens, heads, p)
                for name, x, y in zip(('ctx', 'lse', 'dqkv'), a, b):
                    if not torch.equal(x, y):
                        diff = (x != y) | torch.isnan(y.float())
                        bad.append((mode, variant[0], p, name, int(diff.sum()), diff.nonzero()[0].tolist(), bool(torch.isfinite(y.float()).all())))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ax.MODES)
def test_zero_length_utterance(ops, mode):
    """S3: the rows of the utterance of length 0 are exactly zero in ctx, lse and dqkv (p = 0 and p = 0.1), and at p = 0 the other utterances
    are bit for bit what they are in a batch without it"""
    N, lens, heads = ax.SHAPES['S3']['N'], ax.SHAPES['S3']['lens'], 2
    qkv, dctx = ax.round_inputs(mode, *ax.make_inputs('randn', N, lens, heads))
    others = [b for b, n in enumerate(lens) if n > 0]
    empty = [b for b, n in enumerate(lens) if n == 0]
    assert empty
    with Mode(ops, mode):
        for variant in ax.variants(mode):
            for p in (0.0, 0.1):
                out = run(ops, variant, qkv, dctx, lens, heads, p)
                assert all(bool(torch.isfinite(t.double()).all()) for t in out)
                assert all(not t[b].any() for t in out for b in empty), (mode, variant[0], p)
                assert float(out[2][others].abs().max()) > 0
            alone = run(ops, variant, qkv[others], dctx[others], [lens[b] for b in others], heads, 0.0)
            out = run(ops, variant, qkv, dctx, lens, heads, 0.0)
            assert all(torch.equal(t[others], a) for t, a in zip(out, alone)), (mode, variant[0])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['f32', 'bf16x3', 'bf16'])
def test_powers_of_two_pass_through(ops, mode):
    """bwd(2^k dctx) == 2^k bwd(dctx) and fwd(2^k V).ctx == 2^k fwd(V).ctx for k = +-6 at p = 0.1, bitwise: every rounding in the kernels is
    relative.  (fp16 is exempt: its P and dS operands leave the normal range, DESIGN.md.)"""
    N, lens, heads, p = ax.SHAPES['S1']['N'], ax.SHAPES['S1']['lens'], 2, 0.1
    qkv, dctx = ax.round_inputs(mode, *ax.make_inputs('randn', N, lens, heads))
    D = 64 * heads
    with Mode(ops, mode):
        for variant in ax.variants(mode):
            ctx, lse, dqkv = run(ops, variant, qkv, dctx, lens, heads, p)
            assert float(dqkv.abs().max()) > 0
            for k in (6, -6):
                f = 2.0 ** k
                c2, l2, d2 = run(ops, variant, qkv, dctx * f, lens, heads, p)
                assert torch.equal(c2, ctx) and torch.equal(l2, lse) and torch.equal(d2.double(), dqkv.double() * f), (mode, variant[0], k)
                scaled = qkv.clone()
                scaled[:, :, 2 * D:] *= f
                c3, l3 = forward(ops, variant, scaled, lens, heads, p)
                assert torch.equal(c3.cpu().double(), ctx.double() * f) and torch.equal(l3.cpu(), lse), (mode, variant[0], k)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ax.MODES)
def test_hard_attention_is_exact(ops, mode):
    """Every softmax is exactly 0 / 1/2 / 1 (scores 128 against at most 4; a class's two members sit two key tiles apart, so the running
    maximum is set in one tile and met again, tied, two tiles later): ctx equals float64 exactly in every mode and storage variant; classes
    of one have the exact lse, dq = dk = 0 and dv = their own dO row, bitwise; everything else (the backward of the classes of two goes
    through exp(s - lse) with a rounded lse) is held to its tier-2 bound."""
    N, lens, heads = HARD['N'], HARD['lens'], 2
    qkv, dctx = ax.hard_inputs(N, lens, heads)
    assert all(torch.equal(t, ax.round_inputs(mode, t)) for t in (qkv, dctx))
    size = ax.class_size(N, lens)
    one = size == 1
    if mode in ax.H16:                          # base 2: the 16-bit image of q * QSCALE2 times 32, one exact product (:862, :975)
        lse_one = float(torch.tensor(32.0 * ax.QSCALE2).to(ax.H16[mode]).float()) * 32.0
    else:
        lse_one = 128.0
    bad = []
    with Mode(ops, mode):
        for variant in ax.variants(mode):
            name, qdt, cdt, odt = variant
            ctx, lse, dqkv = run(ops, variant, qkv, dctx, lens, heads, 0.0)
            bd = ax.bounds(qkv, dctx, lens, heads, mode, ctx_store=mode if cdt != torch.float32 else None)
            exact = (torch.round(bd['ref']['ctx'] * 8) / 8).float()              # (v + v') / 2 of multiples of 1/4: float64 is off by its own 1e-15
            assert float((exact.double() - bd['ref']['ctx']).abs().max()) < 1e-12 and float(exact.abs().max()) > 0
            if not torch.equal(ctx.float(), exact.to(cdt).float()):
                bad.append((name, 'ctx not exact', float((ctx.double() - bd['ref']['ctx']).abs().max())))
            got = as_dict(mode, ctx, lse, dqkv)
            if not bool((lse.transpose(1, 2)[one] == lse_one).all()):
                bad.append((name, 'lse of the classes of one', lse.transpose(1, 2)[one].unique().tolist()[:4], lse_one))
            if got['dq'][one].any() or got['dk'][one].any():
                bad.append((name, 'dq / dk of the classes of one not zero'))
            if not torch.equal(got['dv'][one].float(), dctx[one]):
                bad.append((name, 'dv of the classes of one'))
            miss, ratios = ax.check_all(got, bd, lens, dict(ctx=cdt, dq=odt, dk=odt, dv=odt), tag=f'hard {mode} ({name})')
            print(f'[hard] {mode} ({name}): measured / bound ' + ' '.join(f'{n}={ratios[n]:.3g}' for n in ax.NAMES))
            bad += miss
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------------------
# tier 2: every element against its a-priori bound
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('mode', ax.MODES)
@pytest.mark.parametrize('kind', ax.KINDS)
def test_every_element_within_its_bound(ops, kind, mode):
    """ctx, lse, dq, dk, dv of every storage variant at S1 and S2 (and S4, renumbered workgroups, for 'last'), p = 0 and p = 0.1 under the
    host mask: every valid element inside its bound, padded rows exactly zero, nothing excluded"""
    bad = []
    with Mode(ops, mode):
        for sname in ('S1', 'S2') + (('S4',) if kind == 'last' else ()):
            N, lens, heads = ax.SHAPES[sname]['N'], ax.SHAPES[sname]['lens'], 2
            qkv, dctx = ax.round_inputs(mode, *ax.make_inputs(kind, N, lens, heads))
            for p in (0.0, 0.1):
                keep = host_keep(lens, heads, N, p) if p else None
                cache = {}
                worst = {}
                for variant in ax.variants(mode):
                    name, qdt, cdt, odt = variant
                    store = mode if cdt != torch.float32 else None
                    if store not in cache:
                        cache[store] = ax.bounds(qkv, dctx, lens, heads, mode, keep, p, ctx_store=store)
                    got = as_dict(mode, *run(ops, variant, qkv, dctx, lens, heads, p))
                    miss, ratios = ax.check_all(got, cache[store], lens, dict(ctx=cdt, dq=odt, dk=odt, dv=odt), tag=f'{sname} {kind} {mode} p={p} ({name})')
                    bad += miss
                    worst = {n: max(worst.get(n, 0.0), ratios[n]) for n in ratios}
                print(f'[bound] {mode} {kind} {sname} p={p}: measured / bound ' + ' '.join(f'{n}={worst[n]:.3g}' for n in ax.NAMES))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ax.MODES)
@pytest.mark.parametrize('kind', ['peaked', 'rising', 'last'])
def test_probabilities_read_out_of_the_forward_and_of_dkv(ops, kind, mode):
    """The probabilities themselves, element by element against the float64 softmax of the rounded operands: out of the forward (V = the
    identity on one key block per pass) and out of the dK/dV kernel (dctx = the identity on one query block per pass, dV is P^T), three
    passes each at S1.  The only place where the dK/dV kernel's recomputed P, and what scaling k instead of q costs, are looked at."""
    N, lens, heads = ax.SHAPES['S1']['N'], ax.SHAPES['S1']['lens'], 2
    D = 64 * heads
    qkv, _ = ax.round_inputs(mode, *ax.make_inputs(kind, N, lens, heads))
    zeros = torch.zeros(len(lens), N, D)
    split = lambda t: t.double().reshape(len(lens), N, heads, 64).transpose(1, 2)
    bad = []
    with Mode(ops, mode):
        for variant in ax.variants(mode):
            name, qdt, cdt, odt = variant
            store = mode if cdt != torch.float32 else None
            Pf, Pb, P = (torch.zeros(len(lens), heads, N, N, dtype=torch.float64) for _ in range(3))
            for j, x in ax.readout_forward_passes(qkv, heads):
                bd = ax.bounds(x, zeros, lens, heads, mode)
                ctx = forward(ops, variant, x, lens, heads, 0.0)[0].cpu()
                miss = ax.between(ctx, bd['ref']['ctx'], bd['bnd']['ctx'], cdt)
                if miss.any():
                    bad.append((mode, name, kind, 'forward', j, int(miss.sum()), ax.ratio(ctx, bd['ref']['ctx'], bd['bnd']['ctx'], cdt)))
                w = min(64, N - 64 * j)
                Pf[..., 64 * j:64 * j + w] = split(ctx)[..., :w]
                P = bd['P']
            ctx, lse = forward(ops, variant, qkv, lens, heads, 0.0)
            ln = torch.tensor(lens, dtype=torch.int32, device=DEV)
            for i, dctx in ax.readout_dkv_passes(N, lens, heads):
                bd = ax.bounds(qkv, dctx, lens, heads, mode, ctx_store=store)
                dqkv = ops.attention_bwd(qkv.to(DEV).to(qdt).contiguous(), ctx, dctx.to(DEV).to(cdt), lse, ln, heads, SEED, 0.0, out_dtype=odt).cpu()
                dv = dqkv[:, :, 2 * D:]
                miss = ax.between(dv, bd['ref']['dv'], bd['bnd']['dv'], odt)
                if miss.any():
                    bad.append((mode, name, kind, 'dK/dV', i, int(miss.sum()), ax.ratio(dv, bd['ref']['dv'], bd['bnd']['dv'], odt)))
                w = min(64, N - 64 * i)
                Pb[:, :, 64 * i:64 * i + w, :] = split(dv)[..., :w].transpose(-1, -2)
            ff, fb = ax.probability_figures(Pf, P), ax.probability_figures(Pb, P)
            print(f'[read-out] {mode} {kind} ({name}): forward max|dP|={ff[0]:.3g} max|dP|/P={ff[1]:.3g};  dK/dV max|dP|={fb[0]:.3g} max|dP|/P={fb[1]:.3g}')
    assert not bad, bad
