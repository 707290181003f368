"""The streaming HiFi-GAN vocoder on the GPU: chunks bitwise equal to the whole call in both operand modes, graph replay against eager
launches, ring wrap-around, the window entry points one by one against their unwindowed forms, stream ownership and
``SpeechSynthesizer.stream``."""
import pytest
import torch

from tests import helpers
from tests import vocoder_helpers as vh
from ubisoft_laforge_daft_exprt_amd import vocoder as voc
from ubisoft_laforge_daft_exprt_amd._lib import lib

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu

# one frame; the network's right reach in frames (13) and one past it (the plan's lookahead); around the chunk sizes: 8, 9 and 27 = 9 F for
# chunks of 3, 8 = F, 9 = F + 1 for chunks of 8, 64 = 2 F and 65 = 2 F + 1 for chunks of 32; 40 / 41 cross several tiles at every stage
LENGTHS = [1, 41, 13, 14, 27, 8, 9, 40, 64, 65]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mels(lengths, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(len(lengths), 80, max(lengths), generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0).to(DEV)


@pytest.fixture(scope='module')
def vocoders():
    sd = vh.state_dict()
    return {p: voc.HiFiGanVocoder(sd, device=DEV, precision=p) for p in ('f32', 'bf16')}


@pytest.fixture(scope='module')
def whole(vocoders):
    """infer_batch on the shared batch, once per operand mode"""
    mels = _mels(LENGTHS)
    return mels, {p: v.infer_batch(mels, LENGTHS)[0] for p, v in vocoders.items()}


def _collect(stream):
    chunks, valid = zip(*list(stream))
    return torch.cat(chunks, dim=1), torch.stack(valid).sum(dim=0)


def _padded(audio, cols):
    out = torch.zeros(audio.shape[0], cols, dtype=audio.dtype, device=audio.device)
    out[:, :min(cols, audio.shape[1])] = audio[:, :cols]
    return out


@pytest.mark.parametrize('chunk_frames', [3, 8, 32])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_streamed_equals_whole_bitwise(vocoders, whole, precision, chunk_frames):
    mels, ref = whole
    s = vocoders[precision].stream(mels, LENGTHS, chunk_frames=chunk_frames)
    assert len(s) == -(-max(LENGTHS) // chunk_frames)
    got, valid = _collect(s)
    assert got.shape == (len(LENGTHS), len(s) * chunk_frames * 256) and got.dtype == torch.float32
    assert torch.equal(got, _padded(ref[precision], got.shape[1])), (precision, chunk_frames)
    assert valid.tolist() == [256 * n for n in LENGTHS]
    assert torch.count_nonzero(got).item() > 0
    with pytest.raises(StopIteration):
        next(s)
    # lengths as a device tensor: the same stream
    got2, _ = _collect(vocoders[precision].stream(mels, torch.tensor(LENGTHS, device=DEV), chunk_frames=chunk_frames))
    assert torch.equal(got, got2)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_replay_equals_eager_and_one_capture_serves_the_stream(vocoders, whole, precision):
    mels, _ = whole
    replayed = vocoders[precision].stream(mels, LENGTHS, chunk_frames=8, use_graph=True)
    eager = vocoders[precision].stream(mels, LENGTHS, chunk_frames=8, use_graph=False)
    a, va = _collect(replayed)
    b, vb = _collect(eager)
    assert torch.equal(a, b) and torch.equal(va, vb)
    assert len(replayed) == 9 and replayed.captures == 1 and replayed.graph is not None
    assert eager.captures == 0 and eager.graph is None
    assert int(replayed.cursor.item()) == 9 and int(eager.cursor.item()) == 9
    single = vocoders[precision].stream(mels[:1, :, :1].contiguous(), [1], chunk_frames=8)
    assert len(list(single)) == 1 and single.captures == 0          # the first chunk never waits for a capture


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_ring_wrap_on_a_long_row(vocoders, precision):
    v = vocoders[precision]
    mel = _mels([300], seed=6)
    ref, _ = v.infer_batch(mel, [300])
    s = v.stream(mel, [300], chunk_frames=32)
    for t in s.plan.tensors.values():
        assert t['ring'] < 300 * t['scale']                         # every ring wraps
    got, valid = _collect(s)
    assert torch.equal(got, _padded(ref, got.shape[1])) and valid.tolist() == [300 * 256]
    short = v.stream(mel[:, :, :65].contiguous(), [65], chunk_frames=32)
    assert s.workspace_bytes == short.workspace_bytes == s.plan.ring_bytes(1) + 32 * 256 * 4 + 4


# ---- the window entry points, one by one --------------------------------------------------------------------------------------------
def _pack(w, up, bf16):
    if up > 1:
        cin, cout, taps = w.shape[0], w.shape[1], 2
    else:
        cout, cin, taps = w.shape
    n = torch.zeros(1, dtype=torch.long)
    lib().dx_voc_pack_size(cout, cin, taps, up, bf16, n.data_ptr())
    buf = torch.empty(int(n.item()), dtype=torch.uint8, device=DEV)
    lib().dx_voc_pack(w.contiguous().data_ptr(), buf.data_ptr(), cout, cin, taps, up, bf16, _stream())
    return buf


def _lens(B, N, scale):
    frames = [max(1, (N // scale) - 3 * b) for b in range(B)]
    return frames, torch.tensor(frames, dtype=torch.int32, device=DEV)


POISON = 7.0


def _ring_of(full, size, a, b):
    """a ring (B, size, C) that holds logical rows [a, b) of ``full`` (B, N, C) at their slots and POISON in every other slot"""
    ring = torch.full((full.shape[0], size, full.shape[2]), POISON, device=DEV)
    n = torch.arange(max(a, 0), min(b, full.shape[1]), device=DEV)
    assert n.numel() <= size
    ring[:, n & (size - 1)] = full[:, n]
    return ring


def _pow2(n):
    return 1 << (n - 1).bit_length()


def _step_windows(launch, ref, valid, N, up, step, lag, left, right, X, R=None, Y0=None):
    """Steps the cursor over the N tile rows.  Before chunk c the X ring (and R's, and for the accumulating modes Y's) is filled with
    exactly the logical rows the window may touch, POISON elsewhere, so a wrong slot or a read outside the reach shows.  After the
    launch the window's rows must equal ``ref`` (the unwindowed entry point's output) bit for bit and every other slot of the Y ring
    must be untouched.  ``launch(Xring, Yring, Rring, cursor, masks...)`` performs the windowed call."""
    B = ref.shape[0]
    cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
    nx, ny, nr = _pow2(step + lag + left + right), _pow2((step + lag) * up), 2 * _pow2((step + lag) * up)
    assert nx < N and ny < N * up
    chunks = max(1, -(-(N - lag) // step))
    seen = torch.zeros(B, N * up, dtype=torch.bool, device=DEV)
    for c in range(chunks):
        lo, hi = (0 if c == 0 else c * step + lag), (c + 1) * step + lag
        Xr = _ring_of(X, nx, lo - left, hi + right) if X.dim() == 3 and X.shape[1] == N else X     # the mel is read in place
        Rr = _ring_of(R, nr, lo * up, hi * up) if R is not None else None
        Yr = _ring_of(Y0, ny, lo * up, hi * up) if Y0 is not None else torch.full((B, ny, ref.shape[2]), POISON, device=DEV)
        before = Yr.clone()
        launch(Xr, Yr, Rr, cursor, nx - 1 if Xr is not X else 0, ny - 1, nr - 1 if Rr is not None else 0)
        lib().dx_voc_stream_advance(cursor.data_ptr(), _stream())
        for b in range(B):
            rows = torch.arange(lo * up, max(lo * up, min(hi * up, valid[b] * up)), device=DEV)     # none once the row has ended
            slots = rows & (ny - 1)
            assert torch.equal(Yr[b, slots], ref[b, rows]), (c, b)
            keep = torch.ones(ny, dtype=torch.bool, device=DEV)
            keep[slots] = False
            assert torch.equal(Yr[b, keep], before[b, keep]), (c, b, 'a store outside the window')
            seen[b, rows] = True
    assert int(cursor.item()) == chunks
    for b in range(B):
        assert bool(seen[b, :valid[b] * up].all())


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C,k,d', [(256, 11, 5), (128, 3, 1)])
def test_conv_win_equals_conv_bitwise(C, k, d, bf16):
    g = torch.Generator().manual_seed(C + k + d)
    B, N, scale, step, lag = 3, 150, 2, 24, 5
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(C, generator=g)).to(DEV)
    Wp = _pack(W, 1, bf16)
    reach = d * (k - 1) // 2
    for mode, resid in ((0, False), (0, True), (1, True), (2, True)):
        Y0 = torch.randn(B, N, C, generator=g).to(DEV)
        Rf = torch.randn(B, N, C, generator=g).to(DEV) if resid else None
        ref = Y0.clone()
        lib().dx_voc_conv(X.data_ptr(), N * C, C, 1, Wp.data_ptr(), bias.data_ptr(), ref.data_ptr(), N * C, Rf.data_ptr() if resid else None,
                          fr.data_ptr(), scale, B, N, C, C, k, d, 1, 1, mode, bf16, _stream())

        def launch(Xr, Yr, Rr, cur, mx, my, mr):
            lib().dx_voc_conv_win(Xr.data_ptr(), Xr.shape[1] * C, C, 1, Wp.data_ptr(), bias.data_ptr(), Yr.data_ptr(), Yr.shape[1] * C,
                                  Rr.data_ptr() if Rr is not None else None, Rr.shape[1] * C if Rr is not None else 0,
                                  fr.data_ptr(), scale, B, N, C, C, k, d, 1, 1, mode, bf16, cur.data_ptr(), step, lag, mx, my, mr, _stream())
        _step_windows(launch, ref, [f * scale for f in frames], N, 1, step, lag, reach, reach, X, Rf, Y0 if mode else None)


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('Cin,u', [(512, 8), (64, 2)])
def test_transposed_conv_win_equals_conv_bitwise(Cin, u, bf16):
    g = torch.Generator().manual_seed(Cin + u)
    Cout, B, N, scale, step, lag = Cin // 2, 3, 70, 1, 9, 4
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, Cin, generator=g).to(DEV)
    W = (torch.randn(Cin, Cout, 2 * u, generator=g) / Cin ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
    Wp = _pack(W, u, bf16)
    ref = torch.full((B, N * u, Cout), POISON, device=DEV)
    lib().dx_voc_conv(X.data_ptr(), N * Cin, Cin, 1, Wp.data_ptr(), bias.data_ptr(), ref.data_ptr(), N * u * Cout, None,
                      fr.data_ptr(), scale, B, N, Cin, Cout, 2, 1, u, 1, 0, bf16, _stream())

    def launch(Xr, Yr, Rr, cur, mx, my, mr):
        lib().dx_voc_conv_win(Xr.data_ptr(), Xr.shape[1] * Cin, Cin, 1, Wp.data_ptr(), bias.data_ptr(), Yr.data_ptr(), Yr.shape[1] * Cout, None, 0,
                              fr.data_ptr(), scale, B, N, Cin, Cout, 2, 1, u, 1, 0, bf16, cur.data_ptr(), step, lag, mx, my, mr, _stream())
    _step_windows(launch, ref, frames, N, u, step, lag, 1, 1, X)


@pytest.mark.parametrize('bf16', [0, 1])
def test_conv_pre_win_reads_the_mel_in_place(bf16):
    g = torch.Generator().manual_seed(11)
    B, T, N, step, lag = 3, 90, 77, 12, 11
    frames, fr = [77, 1, 50], torch.tensor([77, 1, 50], dtype=torch.int32, device=DEV)
    mel = torch.randn(B, 80, T, generator=g).to(DEV)
    W = (torch.randn(512, 80, 7, generator=g) / (80 * 7) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(512, generator=g)).to(DEV)
    Wp = _pack(W, 1, bf16)
    ref = torch.empty(B, N, 512, device=DEV)
    lib().dx_voc_conv(mel.data_ptr(), 80 * T, 1, T, Wp.data_ptr(), bias.data_ptr(), ref.data_ptr(), N * 512, None,
                      fr.data_ptr(), 1, B, N, 80, 512, 7, 1, 1, 0, 0, bf16, _stream())

    def launch(Xr, Yr, Rr, cur, mx, my, mr):
        assert Xr is mel and mx == 0
        lib().dx_voc_conv_win(mel.data_ptr(), 80 * T, 1, T, Wp.data_ptr(), bias.data_ptr(), Yr.data_ptr(), Yr.shape[1] * 512, None, 0,
                              fr.data_ptr(), 1, B, N, 80, 512, 7, 1, 1, 0, 0, bf16, cur.data_ptr(), step, lag, 0, my, 0, _stream())
    _step_windows(launch, ref, frames, N, 1, step, lag, 3, 3, mel)


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C,k,d', [(64, 11, 5), (32, 3, 1)])
def test_pair_win_equals_pair_bitwise(C, k, d, bf16):
    g = torch.Generator().manual_seed(C * 7 + k * 3 + d)
    B, N, scale, step, lag = 3, 200, 4, 20, 9
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W1 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    W2 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    b1, b2 = (0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    P1, P2 = _pack(W1, 1, bf16), _pack(W2, 1, bf16)
    reach = (d + 1) * (k - 1) // 2
    for mode in (0, 1, 2):
        Y0 = torch.randn(B, N, C, generator=g).to(DEV)
        ref = Y0.clone()
        lib().dx_voc_pair(X.data_ptr(), N * C, P1.data_ptr(), b1.data_ptr(), P2.data_ptr(), b2.data_ptr(), ref.data_ptr(),
                          fr.data_ptr(), scale, B, N, C, k, d, mode, bf16, _stream())

        def launch(Xr, Yr, Rr, cur, mx, my, mr):
            lib().dx_voc_pair_win(Xr.data_ptr(), Xr.shape[1] * C, P1.data_ptr(), b1.data_ptr(), P2.data_ptr(), b2.data_ptr(), Yr.data_ptr(),
                                  Yr.shape[1] * C, fr.data_ptr(), scale, B, N, C, k, d, mode, bf16, cur.data_ptr(), step, lag, mx, my, _stream())
        _step_windows(launch, ref, [f * scale for f in frames], N, 1, step, lag, reach, reach, X, None, Y0 if mode else None)


def test_post_win_equals_post_bitwise():
    g = torch.Generator().manual_seed(12)
    B, N, scale, step = 3, 300, 4, 70
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, 32, generator=g).to(DEV)
    W = (torch.randn(1, 32, 7, generator=g) / 8).to(DEV)
    bias = torch.tensor([0.05], device=DEV)
    chunks = -(-N // step)
    ref = torch.full((B, chunks * step), 3.0, device=DEV)
    lib().dx_voc_post(X.data_ptr(), N * 32, W.data_ptr(), bias.data_ptr(), ref.data_ptr(), chunks * step, fr.data_ptr(), scale, B, N, chunks * step, _stream())
    cursor = torch.zeros(1, dtype=torch.int32, device=DEV)
    nx = _pow2(step + 6)
    assert nx < N
    for c in range(chunks):
        Xr = _ring_of(X, nx, c * step - 3, (c + 1) * step + 3)
        Y = torch.full((B, step + 2), 3.0, device=DEV)
        lib().dx_voc_post_win(Xr.data_ptr(), nx * 32, W.data_ptr(), bias.data_ptr(), Y.data_ptr(), step + 2, fr.data_ptr(), scale, B, N, step,
                              cursor.data_ptr(), step, 0, nx - 1, 0, _stream())
        lib().dx_voc_stream_advance(cursor.data_ptr(), _stream())
        assert torch.equal(Y[:, :step], ref[:, c * step:(c + 1) * step]), c       # zeros at and past each row's end included
        assert bool((Y[:, step:] == 3.0).all())
    assert torch.count_nonzero(ref[0, :N]).item() > 0


# ---- ownership ------------------------------------------------------------------------------------------------------------------------
def test_streams_own_their_state(vocoders, whole):
    mels, ref = whole
    v = vocoders['f32']
    other = _mels([20, 33], seed=8)
    ref_other, _ = v.infer_batch(other, [20, 33])
    a, b = v.stream(mels, LENGTHS, chunk_frames=8), v.stream(other, [20, 33], chunk_frames=8)
    ca, cb = [], []
    for i in range(len(a)):                                          # interleaved: a, b, a, b, ... until b ends, then a alone
        ca.append(next(a)[0])
        if i < len(b):
            cb.append(next(b)[0])
    ga, gb = torch.cat(ca, dim=1), torch.cat(cb, dim=1)
    assert torch.equal(ga, _padded(ref['f32'], ga.shape[1])) and torch.equal(gb, _padded(ref_other, gb.shape[1]))
    # a stream abandoned after two chunks leaves nothing behind: a fresh one gives the whole result
    dropped = v.stream(mels, LENGTHS, chunk_frames=8)
    next(dropped), next(dropped)
    del dropped
    got, _ = _collect(v.stream(mels, LENGTHS, chunk_frames=8))
    assert torch.equal(got, ga)
    # clone=False: the stream's own buffer on every step
    s = v.stream(other, [20, 33], chunk_frames=8, clone=False)
    ptrs, parts = set(), []
    for audio, _ in s:
        ptrs.add(audio.data_ptr())
        parts.append(audio.clone())
    assert len(ptrs) == 1 and torch.equal(torch.cat(parts, dim=1), gb)


def test_speech_synthesizer_stream(vocoders):
    import ubisoft_laforge_daft_exprt_amd as dx
    case = helpers.load_case('inference_add')
    hp = helpers.golden_hparams(stats={'spk 0': {'energy': {'mean': 2.0, 'std': 1.5}, 'pitch': {'mean': 5.0, 'std': 0.25}},
                                       'spk 1': {'energy': {'mean': 1.7, 'std': 1.1}, 'pitch': {'mean': 4.6, 'std': 0.3}}})
    dx.set_precision('f32')
    model = dx.DaftExprt(hp).to(DEV)
    model.load_state_dict(helpers.golden_state_dict(), strict=True)
    synth = dx.SpeechSynthesizer(model.eval(), hp, vocoders['f32'])

    def args():
        t = lambda k: torch.from_numpy(case[k]).clone().to(DEV)
        inputs = (t('in/symbols'), t('in/dur_factors'), t('in/energy_factors'), t('in/pitch_factors'), t('in/input_lengths'), t('in/speaker_ids'))
        prosody = {k: t('in/prosody_' + k) for k in ('duration_preds', 'durations_int', 'energy_preds', 'pitch_preds')}
        return inputs, 'add', prosody, t('in/spk_embs'), t('in/accent_emb')
    ref = synth(*args())
    for use_graph in (True, False):
        out = synth.stream(*args(), use_graph=use_graph, chunk_frames=8)
        assert set(out) == {'chunks', 'sample_lengths', 'mel', 'output_lengths', 'encoder_preds', 'weights'}
        assert torch.equal(out['mel'], ref['mel']) and torch.equal(out['output_lengths'], ref['output_lengths'])
        assert torch.equal(out['sample_lengths'], ref['sample_lengths'])
        assert len(out['chunks']) == -(-int(ref['output_lengths'].max()) // 8)
        pcm, audio, valid = zip(*list(out['chunks']))
        pcm, audio = torch.cat(pcm, dim=1), torch.cat(audio, dim=1)
        assert pcm.dtype == torch.int16 and torch.equal(pcm, _padded(ref['pcm'], pcm.shape[1])), use_graph
        assert torch.equal(audio, _padded(ref['audio'], audio.shape[1]))
        assert torch.equal(torch.stack(valid).sum(dim=0), ref['sample_lengths'])
        assert pcm.abs().max().item() > 0
    out = synth.stream(*args(), pcm16=False, chunk_frames=8)
    assert all(p is None for p, _, _ in out['chunks'])
