"""The vocoder's 'bf16x3' precision (split-bf16 operands, operand mode 2) on the GPU.

1. Single launches through the C ABI on integer operands that the split represents exactly: the result is the float64 result, bit for
   bit, in every conv form and in the fused pair; the same operands in bf16 mode are not.
2. One conv and one pair on randn against float64, element-wise, inside the mode's worst-case error bound.
3. The whole generators against the reference's waveforms: no further from them than the f32 mode plus 1/64 of the bf16 mode's error.
4. The bitwise properties of the other modes: batch rows, repeated calls, chunking, streaming."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vocoder_helpers as vh
from ubisoft_laforge_daft_exprt_amd import vocoder as voc
from ubisoft_laforge_daft_exprt_amd._lib import lib

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
CONFIGS = {'v1': voc.v1_config, 'v2': voc.v2_config, 'v3': voc.v3_config}
X3 = 2                         # the C ABI's operand mode
N, LENS = 70, (70, 23)         # one full 64-sample tile and a 6-sample tail; the second row ends inside the first tile
POISON = 7.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack(w, up, mode):
    if up > 1:
        cin, cout, taps = w.shape[0], w.shape[1], 2
    else:
        cout, cin, taps = w.shape
    n = torch.zeros(1, dtype=torch.long)
    lib().dx_voc_pack_size(cout, cin, taps, up, mode, n.data_ptr())
    buf = torch.empty(int(n.item()), dtype=torch.uint8, device=DEV)
    lib().dx_voc_pack(w.to(DEV).contiguous().data_ptr(), buf.data_ptr(), cout, cin, taps, up, mode, _stream())
    return buf


def _frames():
    return torch.tensor(LENS, dtype=torch.int32, device=DEV)


# ---- 1. exact launches ----------------------------------------------------------------------------------------------------------
def _wide(g, shape, lo=-3):
    """256 p + q, p and q in lo..3: ten significant bits, so bf16 keeps hi != x and lo != 0 for most values"""
    return 256 * torch.randint(lo, 4, shape, generator=g) + torch.randint(lo, 4, shape, generator=g)


def _check_exact_operands(*tensors):
    """every operand is an integer of at most 16 significant bits: hi + lo is the operand exactly (int64 arithmetic)"""
    for t in tensors:
        assert t.dtype == torch.int64
        a = t.abs()
        odd = a // torch.clamp(a & -a, min=1)           # a without its trailing zero bits
        assert int(odd.max()) < 1 << 16, int(odd.max())


def _conv_ref(x, w, bias, d, up):
    """x (Cin, n), w as torch holds it -> (n up, Cout); the dtype of its arguments (int64: via float64, exact below 2^53)"""
    if up > 1:
        return F.conv_transpose1d(x[None].double(), w.double(), bias.double(), stride=up, padding=up // 2)[0].T
    return F.conv1d(x[None].double(), w.double(), bias.double(), padding=d * (w.shape[2] - 1) // 2, dilation=d)[0].T


# (Cin, Cout, taps, dilation, up, mel layout): conv_pre's form on the strided (B, 80, T) input, the two polyphase transposed convs
# (up 8 into 256 columns, up 2 into 16), the widest window (k 11, dilation 5: taps Cin = 2816), a dilated k 3, a 16-column conv
EXACT_CONVS = [(80, 512, 7, 1, 1, True), (512, 256, 2, 1, 8, False), (32, 16, 2, 1, 2, False), (256, 256, 11, 5, 1, False),
               (128, 128, 3, 3, 1, False), (16, 16, 3, 3, 1, False)]


def _exact_conv_case(shape, wide_x, seed):
    Cin, Cout, k, d, up, mel = shape
    g = torch.Generator().manual_seed(seed)
    B = len(LENS)
    x = _wide(g, (B, Cin, N)) if wide_x else torch.randint(-2, 3, (B, Cin, N), generator=g)              # set (a) / set (b)
    wshape = (Cin, Cout, 2 * up) if up > 1 else (Cout, Cin, k)
    w = torch.randint(-2, 3, wshape, generator=g) if wide_x else _wide(g, wshape)
    bias = torch.randint(-100, 101, (Cout,), generator=g)
    res = torch.randint(-1000, 1001, (B, N * up, Cout), generator=g)
    y0 = torch.randint(-1000, 1001, (B, N * up, Cout), generator=g)
    _check_exact_operands(x, w, bias, res, y0)
    # every partial sum, in any order, is below sum |x| |w| + |bias| + |res| + |y0|: an integer below 2^24 is exact in fp32
    mag = max(float(_conv_ref(x[b].abs(), w.abs(), bias.abs(), d, up).max()) for b in range(B)) + 2000
    assert mag < 2 ** 24 and (k if up == 1 else 2) * Cin <= 2816, mag
    return x, w, bias, res, y0


def _run_conv(shape, x, w, bias, res, y0, acc_mode, mode):
    Cin, Cout, k, d, up, mel = shape
    B = len(LENS)
    X = (x if mel else x.transpose(1, 2)).float().contiguous().to(DEV)
    strides = (Cin * N, 1, N) if mel else (N * Cin, Cin, 1)
    Wp, bd, R = _pack(w.float(), up, mode), bias.float().to(DEV), res.float().to(DEV)
    Y = y0.float().to(DEV) if acc_mode else torch.full((B, N * up, Cout), POISON, device=DEV)
    lib().dx_voc_conv(X.data_ptr(), *strides, Wp.data_ptr(), bd.data_ptr(), Y.data_ptr(), N * up * Cout, R.data_ptr() if acc_mode else None,
                      _frames().data_ptr(), 1, B, N, Cin, Cout, 2 if up > 1 else k, d, up, 0, acc_mode, mode, _stream())
    return Y.cpu().double()


def _want_conv(shape, x, w, bias, res, y0, acc_mode):
    Cin, Cout, k, d, up, mel = shape
    want = torch.zeros(len(LENS), N * up, Cout, dtype=torch.float64)
    for b, n in enumerate(LENS):
        v = _conv_ref(x[b, :, :n], w, bias, d, up)
        want[b, :n * up] = v + (res[b, :n * up] + y0[b, :n * up] if acc_mode else 0)
    return want


@pytest.mark.parametrize('wide_x', [True, False], ids=['set_a', 'set_b'])
@pytest.mark.parametrize('shape', EXACT_CONVS, ids=lambda s: 'x'.join(str(int(v)) for v in s))
def test_conv_is_exactly_float64_on_operands_the_split_represents(shape, wide_x):
    """Set (a): wide activations, small weights -- the result is exact only if lo_a * hi_b is added; set (b), the mirror, only if
    hi_a * lo_b is.  acc_mode 0, and 1 with an integer residual; rows past each batch row's end are written as 0."""
    case = _exact_conv_case(shape, wide_x, seed=sum(shape) + wide_x)
    for acc_mode in (0, 1):
        got, want = _run_conv(shape, *case, acc_mode, X3), _want_conv(shape, *case, acc_mode)
        bad = (got != want).sum().item()
        print(f'{shape} {"a" if wide_x else "b"} acc_mode {acc_mode}: {bad} of {want.numel()} differ, max |diff| {(got - want).abs().max().item():g}')
        assert torch.equal(got, want), (shape, wide_x, acc_mode, bad)
        for b, n in enumerate(LENS):
            assert torch.count_nonzero(got[b, n * shape[4]:]).item() == 0 and torch.count_nonzero(got[b, :n * shape[4]]).item() > 0


def test_the_exact_operands_tell_the_modes_apart():
    """Set (a) in bf16 mode is NOT the float64 result (the activations lose their low bits), and in f32 mode it is."""
    shape = EXACT_CONVS[4]
    case = _exact_conv_case(shape, True, seed=sum(shape) + 1)
    want = _want_conv(shape, *case, 0)
    assert not torch.equal(_run_conv(shape, *case, 0, 1), want)
    assert torch.equal(_run_conv(shape, *case, 0, 0), want)
    assert torch.equal(_run_conv(shape, *case, 0, X3), want)


@pytest.mark.parametrize('C,k,d', [(64, 11, 5), (32, 7, 3), (16, 3, 1)])
def test_pair_is_exactly_float64_on_operands_the_split_represents(C, k, d):
    """The pair's leaky-ReLUs cannot be switched off, so everything is non-negative.  conv1: small x, wide w1 (two non-zeros per output
    channel: the intermediate stays below 2^13) -- exact only with hi_a * lo_b; conv2: the wide intermediate, split when it is written
    to LDS, and small w2 -- exact only with lo_a * hi_b."""
    g = torch.Generator().manual_seed(C + k + d)
    B = len(LENS)
    x = torch.randint(0, 4, (B, C, N), generator=g)
    w1 = torch.zeros(C, C * k, dtype=torch.int64)
    for n in range(C):
        idx = torch.randperm(C * k, generator=g)[:2]
        w1[n, idx] = _wide(g, (2,), lo=0)
    w1 = w1.view(C, C, k)
    w2 = torch.randint(0, 3, (C, C, k), generator=g)
    b1, b2 = torch.randint(0, 101, (C,), generator=g), torch.randint(0, 101, (C,), generator=g)
    y0 = torch.randint(0, 1001, (B, N, C), generator=g)
    _check_exact_operands(x, w1, w2, b1, b2, y0)
    want = {0: torch.zeros(B, N, C, dtype=torch.float64), 1: torch.zeros(B, N, C, dtype=torch.float64)}
    for b, n in enumerate(LENS):
        mid = _conv_ref(x[b, :, :n], w1, b1, d, 1)                       # >= 0: the leaky-ReLU is the identity
        assert 0 <= float(mid.min()) and float(mid.max()) < 2 ** 13 and float(w1.max()) > 256
        _check_exact_operands(mid.long())
        v = _conv_ref(mid.T, w2, b2, 1, 1) + x[b, :, :n].T
        assert float(v.max()) + 1000 < 2 ** 24
        want[0][b, :n], want[1][b, :n] = v, v + y0[b, :n]
    X = x.transpose(1, 2).float().contiguous().to(DEV)
    P1, P2 = _pack(w1.float(), 1, X3), _pack(w2.float(), 1, X3)
    b1d, b2d = b1.float().to(DEV), b2.float().to(DEV)
    for acc_mode in (0, 1):
        Y = y0.float().to(DEV) if acc_mode else torch.full((B, N, C), POISON, device=DEV)
        lib().dx_voc_pair(X.data_ptr(), N * C, P1.data_ptr(), b1d.data_ptr(), P2.data_ptr(), b2d.data_ptr(), Y.data_ptr(),
                          _frames().data_ptr(), 1, B, N, C, k, d, acc_mode, X3, _stream())
        got = Y.cpu().double()
        print(f'pair C {C} k {k} d {d} acc_mode {acc_mode}: {(got != want[acc_mode]).sum().item()} differ, max |diff| {(got - want[acc_mode]).abs().max().item():g}')
        assert torch.equal(got, want[acc_mode]), (C, k, d, acc_mode)
        for b, n in enumerate(LENS):
            assert torch.count_nonzero(got[b, n:]).item() == 0 and torch.count_nonzero(got[b, :n]).item() > 0


# ---- 2. random operands, worst-case bound ---------------------------------------------------------------------------------------
U_SPLIT, U_F32 = 3 * 2.0 ** -16, 2.0 ** -24


def _bound(mag, n):
    """|y - y64| <= (3 2^-16 + (n + 8) 2^-24) sum |a| |w|: a = hi + lo + r, |r| <= 2^-16 |a|, for both operands, and lo_a lo_b <=
    2^-16 |a| |b| is dropped (3 2^-16); n products and a handful of epilogue terms accumulate in fp32 ((n + 8) 2^-24)."""
    return (U_SPLIT + (n + 8) * U_F32) * mag


def test_conv_on_randn_is_inside_the_worst_case_bound():
    g = torch.Generator().manual_seed(21)
    C, k, d, B = 256, 11, 5, len(LENS)
    x = torch.randn(B, N, C, generator=g)
    w = torch.randn(C, C, k, generator=g) / (C * k) ** 0.5
    bias = 0.1 * torch.randn(C, generator=g)
    X, bd, Wp = x.to(DEV), bias.to(DEV), _pack(w, 1, X3)
    Y = torch.full((B, N, C), POISON, device=DEV)
    lib().dx_voc_conv(X.data_ptr(), N * C, C, 1, Wp.data_ptr(), bd.data_ptr(), Y.data_ptr(), N * C, None,
                      _frames().data_ptr(), 1, B, N, C, C, k, d, 1, 1, 0, X3, _stream())
    got = Y.cpu().double()
    a = torch.where(x > 0, x, x * torch.tensor(0.1, dtype=torch.float32))          # the prologue as the kernel computes it, in fp32
    for b, n in enumerate(LENS):
        y64 = _conv_ref(a[b, :n].T, w, bias, d, 1)
        mag = _conv_ref(a[b, :n].T.abs(), w.abs(), bias.abs(), d, 1)               # sum |a| |w| (+ |bias|: the bias is a term too)
        err, bound = (got[b, :n] - y64).abs(), _bound(mag, k * C)
        print(f'conv row {b}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}')
        assert bool((err <= bound).all()), (b, (err / bound).max().item())
        assert torch.count_nonzero(got[b, n:]).item() == 0


def test_pair_on_randn_is_inside_the_worst_case_bound():
    """The bound of one conv, applied twice: the intermediate m = lrelu(conv1 + b1) carries conv1's bound dm (the leaky-ReLU has slope
    <= 1, and its own fp32 rounding is one of the + 8 terms), which conv2 passes on as sum |w2| dm; conv2's own error is its bound on
    operands of magnitude |m64| + dm, with b2 and the residual x as terms."""
    g = torch.Generator().manual_seed(22)
    C, k, d, B = 64, 11, 5, len(LENS)
    x = torch.randn(B, N, C, generator=g)
    w1, w2 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5 for _ in range(2))
    b1, b2 = 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    X, b1d, b2d = x.to(DEV), b1.to(DEV), b2.to(DEV)
    P1, P2 = _pack(w1, 1, X3), _pack(w2, 1, X3)
    Y = torch.full((B, N, C), POISON, device=DEV)
    lib().dx_voc_pair(X.data_ptr(), N * C, P1.data_ptr(), b1d.data_ptr(), P2.data_ptr(), b2d.data_ptr(),
                      Y.data_ptr(), _frames().data_ptr(), 1, B, N, C, k, d, 0, X3, _stream())
    got = Y.cpu().double()
    a = torch.where(x > 0, x, x * torch.tensor(0.1, dtype=torch.float32))
    zero = torch.zeros(C)
    for b, n in enumerate(LENS):
        m64 = F.leaky_relu(_conv_ref(a[b, :n].T, w1, b1, d, 1), 0.1)
        dm = _bound(_conv_ref(a[b, :n].T.abs(), w1.abs(), b1.abs(), d, 1), k * C)
        y64 = _conv_ref(m64.T, w2, b2, 1, 1) + x[b, :n].double()
        mag = _conv_ref((m64.abs() + dm).T, w2.abs(), b2.abs(), 1, 1) + x[b, :n].double().abs()
        bound = _conv_ref(dm.T, w2.abs(), zero, 1, 1) + _bound(mag, k * C)
        err = (got[b, :n] - y64).abs()
        print(f'pair row {b}: max err {err.max().item():.3e}, max err / bound {(err / bound).max().item():.3f}')
        assert bool((err <= bound).all()), (b, (err / bound).max().item())
        assert torch.count_nonzero(got[b, n:]).item() == 0


# ---- 3. the whole generator against the reference's waveforms ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def vocoders():
    made = {}

    def get(name, precision):
        if (name, precision) not in made:
            made[name, precision] = voc.HiFiGanVocoder(vh.state_dict(name), config=CONFIGS[name](), device=DEV, precision=precision)
        return made[name, precision]
    return get


def _golden(name):
    if name == 'v1':
        return vh.golden()
    gold = vh.variant_golden(name)
    return gold['lengths'], gold['mels'], gold['wavs']


@pytest.mark.parametrize('name', ['v1', 'v2', 'v3'])
def test_no_further_from_the_reference_than_f32_plus_a_64th_of_bf16(vocoders, name):
    """Per product the bf16 mode perturbs by up to 2 2^-8 and the split by up to 3 2^-16, 1/171 of it; the bar is 1/64 of the bf16
    mode's error on top of the fp32 floor the f32 mode shows, all three measured against the reference's waveform in this run."""
    lengths, mels, wavs = _golden(name)
    assert sorted(lengths) == [1, 13, 40]
    for n, mel, ref in zip(lengths, mels, wavs):
        e = {}
        for p in ('f32', 'bf16', 'bf16x3'):
            err = np.abs(vocoders(name, p).infer(mel).astype(np.float64) - ref.astype(np.float64))
            e[p] = (err.max(), err.mean())
        print(f'{name}, {n} frames, |y - reference| max / mean: ' + ', '.join(f'{p} {e[p][0]:.3e} / {e[p][1]:.3e}' for p in e))
        for norm in (0, 1):
            assert e['bf16x3'][norm] <= e['f32'][norm] + e['bf16'][norm] / 64, (name, n, norm, e)


# ---- 4. bitwise properties ----------------------------------------------------------------------------------------------------------
BATCH = (40, 13, 1)


def _mels(lengths, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(len(lengths), 80, max(lengths), generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0).to(DEV)


@pytest.mark.parametrize('name', ['v1', 'v2', 'v3'])
def test_batch_rows_repeats_and_chunks_are_bitwise_the_utterance_alone(vocoders, name):
    v, mels = vocoders(name, 'bf16x3'), _mels(BATCH)
    assert len(v.topology) == {'v1': 60, 'v2': 42, 'v3': 23}[name]
    audio, slen = v.infer_batch(mels, list(BATCH))
    assert audio.shape == (len(BATCH), 256 * max(BATCH)) and slen == [256 * n for n in BATCH]
    for b, n in enumerate(BATCH):
        alone, _ = v.infer_batch(mels[b:b + 1, :, :n].contiguous(), [n])
        assert torch.equal(audio[b, :256 * n], alone[0]), (name, b, n)
        assert torch.count_nonzero(audio[b, 256 * n:]).item() == 0 and torch.count_nonzero(alone[0]).item() > 0
    again, _ = v.infer_batch(mels, list(BATCH))
    assert torch.equal(audio, again)
    bound = max(BATCH) * voc.workspace_bytes_per_frame(v.config)           # every chunk is one utterance
    chunked, _ = v.infer_batch(mels, list(BATCH), max_workspace_bytes=bound)
    assert torch.equal(audio, chunked)
    other = vocoders(name, 'f32').infer_batch(mels, list(BATCH))[0]
    assert not torch.equal(audio, other)                                      # the mode is its own arithmetic, not the f32 kernels


@pytest.mark.parametrize('name', ['v1', 'v3'])
def test_streamed_in_the_smallest_chunks_equals_whole_bitwise(vocoders, name):
    v, lengths = vocoders(name, 'bf16x3'), [40, 13]
    mels = _mels(lengths, seed=6)
    ref, _ = v.infer_batch(mels, lengths)
    s = v.stream(mels, lengths, chunk_frames=1)                               # stream_plan's smallest: one frame, 256 samples a step
    assert len(s) == 40 and s.plan.launches == voc.stream_plan(v.config, 1, 'f32').launches
    chunks, valid = zip(*list(s))
    got = torch.cat(chunks, dim=1)
    assert got.shape == ref.shape and torch.equal(got, ref), name
    assert torch.stack(valid).sum(dim=0).tolist() == [256 * n for n in lengths] and s.captures == 1


def test_generator_module_is_infer_batch_and_has_no_gradients(vocoders):
    sd = vh.state_dict()
    module = voc.HiFiGANGenerator(precision='bf16x3')
    module.load_state_dict(sd, strict=True)
    module = module.to(DEV)
    mels = _mels(BATCH)
    want, _ = vocoders('v1', 'bf16x3').infer_batch(mels, list(BATCH))
    with torch.no_grad():
        got = module(mels, list(BATCH))
    assert got.shape == (len(BATCH), 1, 256 * max(BATCH)) and torch.equal(got[:, 0], want)
    with pytest.raises(RuntimeError, match="gradients exist for precision 'f32' only, got 'bf16x3'"):
        module(mels, list(BATCH))
