"""The HiFi-GAN V2 and V3 generators on the GPU: parity with the reference fixture (f32), bf16 against f32 at the reference's own
all-bfloat16 figure, batch rows and streamed chunks bitwise equal to the utterance alone, the narrow (16-column) launches and the fused
ResBlock2 chain against F.conv1d and against the two-conv path, and ``SpeechSynthesizer`` with a V3 vocoder.  1, 13 and 40 frames
throughout: at 40 frames every stage has interior, edge and partial 64-sample tiles, and V3's 36-row halo is crossed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers
from tests import vocoder_helpers as vh
from ubisoft_laforge_daft_exprt_amd import vocoder as voc
from ubisoft_laforge_daft_exprt_amd._lib import lib

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu
CONFIGS = {'v2': voc.v2_config, 'v3': voc.v3_config}
BATCH = (40, 13, 1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def vocoders():
    return {(n, p): voc.HiFiGanVocoder(vh.state_dict(n), config=CONFIGS[n](), device=DEV, precision=p)
            for n in vh.VARIANTS for p in ('f32', 'bf16')}


@pytest.fixture(scope='module')
def batch():
    """{name: (mels (3, 80, 40) of lengths (40, 13, 1) from the fixture, zero past each row's end)}"""
    out = {}
    for name in vh.VARIANTS:
        gold = vh.variant_golden(name)
        mels = torch.zeros(len(BATCH), 80, max(BATCH))
        for b, n in enumerate(BATCH):
            mels[b, :, :n] = torch.from_numpy(gold['mels'][gold['lengths'].index(n)])
        out[name] = mels.to(DEV)
    return out


@pytest.fixture(scope='module')
def whole(vocoders, batch):
    """infer_batch on the shared batch, once per configuration and operand mode"""
    return {key: v.infer_batch(batch[key[0]], list(BATCH))[0] for key, v in vocoders.items()}


@pytest.mark.parametrize('name', vh.VARIANTS)
def test_f32_matches_reference_golden(vocoders, name):
    gold = vh.variant_golden(name)
    for n, mel, ref in zip(gold['lengths'], gold['mels'], gold['wavs']):
        got = vocoders[name, 'f32'].infer(mel)
        err = np.abs(got - ref)
        print(f'{name} f32 vs reference, {n} frames: max {err.max():.2e} mean {err.mean():.2e}')
        assert got.shape == ref.shape
        assert err.max() <= 1e-5 and err.mean() <= 1e-6, (n, err.max(), err.mean())


@pytest.mark.parametrize('name', vh.VARIANTS)
def test_bf16_against_f32_snr_is_at_the_all_bfloat16_reference(vocoders, name):
    """Only the MFMA operands are rounded here (activations, residuals and sums stay fp32), so the SNR against the f32 mode is no lower
    than that of the reference run wholly in bfloat16 against its fp64 run (the fixture's figure), less 1 dB for the summation order."""
    gold = vh.variant_golden(name)
    for n, mel, floor in zip(gold['lengths'], gold['mels'], gold['bf16_snr_db']):
        a = vocoders[name, 'f32'].infer(mel).astype(np.float64)
        b = vocoders[name, 'bf16'].infer(mel).astype(np.float64)
        snr = 10 * np.log10((a ** 2).sum() / max(((a - b) ** 2).sum(), 1e-30))
        print(f'{name} bf16 vs f32, {n} frames: SNR {snr:.1f} dB (all-bfloat16 reference {floor:.1f} dB)')
        assert snr >= floor - 1.0, (n, snr, floor)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('name', vh.VARIANTS)
def test_batch_rows_equal_utterances_alone_bitwise(vocoders, batch, whole, name, precision):
    v, mels, audio = vocoders[name, precision], batch[name], whole[name, precision]
    assert audio.shape == (len(BATCH), 256 * max(BATCH))
    for b, n in enumerate(BATCH):
        alone, _ = v.infer_batch(mels[b:b + 1, :, :n].contiguous(), [n])
        assert torch.equal(audio[b, :256 * n], alone[0]), (name, precision, b, n)
        assert torch.count_nonzero(audio[b, 256 * n:]).item() == 0
        assert torch.count_nonzero(alone[0]).item() > 0
    bound = max(BATCH) * voc.workspace_bytes_per_frame(v.config)       # one utterance of 40 frames: every chunk is one utterance
    chunked, slen = v.infer_batch(mels, list(BATCH), max_workspace_bytes=bound)
    assert torch.equal(audio, chunked) and slen == [256 * n for n in BATCH]


def _collect(stream):
    chunks, valid = zip(*list(stream))
    return torch.cat(chunks, dim=1), torch.stack(valid).sum(dim=0)


@pytest.mark.parametrize('chunk_frames', [4, 32])
@pytest.mark.parametrize('precision', ['f32', 'bf16'])
@pytest.mark.parametrize('name', vh.VARIANTS)
def test_streamed_equals_whole_bitwise(vocoders, batch, whole, name, precision, chunk_frames):
    v, mels, ref = vocoders[name, precision], batch[name], whole[name, precision]
    sizes = set()
    for use_graph in (True, False):
        s = v.stream(mels, list(BATCH), chunk_frames=chunk_frames, use_graph=use_graph)
        assert len(s) == -(-max(BATCH) // chunk_frames)
        got, valid = _collect(s)
        want = torch.zeros_like(got)
        want[:, :min(got.shape[1], ref.shape[1])] = ref[:, :got.shape[1]]
        assert torch.equal(got, want), (name, precision, chunk_frames, use_graph)
        assert valid.tolist() == [256 * n for n in BATCH] and torch.count_nonzero(got).item() > 0
        assert s.captures == (1 if use_graph and len(s) > 1 else 0)
        sizes.add(s.workspace_bytes)
    short = v.stream(mels[:, :, :13].contiguous(), [13, 13, 1], chunk_frames=chunk_frames)
    sizes.add(short.workspace_bytes)
    assert sizes == {short.plan.ring_bytes(len(BATCH)) + len(BATCH) * chunk_frames * 256 * 4 + 4}      # not a function of the length


# ---- per-kernel checks ------------------------------------------------------------------------------------------------------
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


def _q(t, bf16):
    return t.to(torch.bfloat16).double() if bf16 else t.double()


def _tol(ref, bf16):
    """test_vocoder_gpu.py's per-kernel bound: a few ulps of the operand format times the output's scale"""
    return (2e-2 if bf16 else 2e-5) * max(1.0, ref.abs().max().item())


def _lens(B, N, scale):
    frames = [max(1, (N // scale) - 3 * b) for b in range(B)]
    return frames, torch.tensor(frames, dtype=torch.int32, device=DEV)


def _finish(ref, y0, mode):
    return ref if mode == 0 else y0 + ref if mode == 1 else (y0 + ref) / 3


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C,k,d', [(16, 3, 1), (16, 7, 3), (16, 11, 5), (128, 5, 6), (128, 7, 12), (64, 7, 12), (32, 5, 2)])
def test_dilated_conv_kernel_at_the_new_widths_and_dilations(C, k, d, bf16):
    g = torch.Generator().manual_seed(C * 100 + k * 10 + d)
    B, N, scale = 3, 150, 2
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(C, generator=g)).to(DEV)
    Wp = _pack(W, 1, bf16)
    for mode, resid in ((0, False), (0, True), (2, True)):
        Y0 = torch.randn(B, N, C, generator=g).to(DEV)
        Y = Y0.clone()
        lib().dx_voc_conv(X.data_ptr(), N * C, C, 1, Wp.data_ptr(), bias.data_ptr(), Y.data_ptr(), N * C, X.data_ptr() if resid else None,
                          fr.data_ptr(), scale, B, N, C, C, k, d, 1, 1, mode, bf16, _stream())
        for b in range(B):
            n = frames[b] * scale
            x = _q(F.leaky_relu(X[b, :n].double(), 0.1), bf16)
            ref = F.conv1d(x.T[None], _q(W, bf16), bias.double(), padding=d * (k - 1) // 2, dilation=d)[0].T
            if resid:
                ref = ref + X[b, :n].double()
            ref = _finish(ref, Y0[b, :n].double(), mode)
            assert (Y[b, :n].double() - ref).abs().max().item() <= _tol(ref, bf16), (b, mode)
            assert torch.count_nonzero(Y[b, n:]).item() == 0


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('k,d', [(3, 1), (7, 3), (11, 5)])
def test_fused_pair_kernel_at_16_channels(k, d, bf16):
    g = torch.Generator().manual_seed(k * 3 + d)
    B, N, scale, C = 3, 200, 4, 16
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W1 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    W2 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    b1, b2 = (0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    P1, P2 = _pack(W1, 1, bf16), _pack(W2, 1, bf16)
    for mode in (0, 1, 2):
        Y0 = torch.randn(B, N, C, generator=g).to(DEV)
        Y = Y0.clone()
        lib().dx_voc_pair(X.data_ptr(), N * C, P1.data_ptr(), b1.data_ptr(), P2.data_ptr(), b2.data_ptr(), Y.data_ptr(),
                          fr.data_ptr(), scale, B, N, C, k, d, mode, bf16, _stream())
        for b in range(B):
            n = frames[b] * scale
            x = _q(F.leaky_relu(X[b, :n].double(), 0.1), bf16).T[None]
            t = F.conv1d(x, _q(W1, bf16), b1.double(), padding=d * (k - 1) // 2, dilation=d)
            t = _q(F.leaky_relu(t, 0.1), bf16)
            ref = F.conv1d(t, _q(W2, bf16), b2.double(), padding=(k - 1) // 2)[0].T + X[b, :n].double()
            ref = _finish(ref, Y0[b, :n].double(), mode)
            assert (Y[b, :n].double() - ref).abs().max().item() <= _tol(ref, bf16), (b, mode)
            assert torch.count_nonzero(Y[b, n:]).item() == 0


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('Cin,Cout,u', [(32, 16, 2), (16, 16, 2), (64, 32, 4)])
def test_transposed_conv_kernel_at_the_new_shapes(Cin, Cout, u, bf16):
    g = torch.Generator().manual_seed(Cin + u)
    B, N, scale = 3, 70, 1
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, Cin, generator=g).to(DEV)
    W = (torch.randn(Cin, Cout, 2 * u, generator=g) / Cin ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
    Wp = _pack(W, u, bf16)
    Y = torch.full((B, N * u, Cout), 7.0, device=DEV)
    lib().dx_voc_conv(X.data_ptr(), N * Cin, Cin, 1, Wp.data_ptr(), bias.data_ptr(), Y.data_ptr(), N * u * Cout, None,
                      fr.data_ptr(), scale, B, N, Cin, Cout, 2, 1, u, 1, 0, bf16, _stream())
    for b in range(B):
        n = frames[b] * scale
        x = _q(F.leaky_relu(X[b, :n].double(), 0.1), bf16).T[None]
        ref = F.conv_transpose1d(x, _q(W, bf16), bias.double(), stride=u, padding=u // 2)[0].T
        assert (Y[b, :n * u].double() - ref).abs().max().item() <= _tol(ref, bf16), b
        assert torch.count_nonzero(Y[b, n * u:]).item() == 0


def test_conv_post_kernel_at_16_channels():
    g = torch.Generator().manual_seed(12)
    B, N, ncols, C = 2, 300, 320, 16
    frames, fr = [300 // 4, 20], torch.tensor([300 // 4, 20], dtype=torch.int32, device=DEV)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W = (torch.randn(1, C, 7, generator=g) / 8).to(DEV)
    bias = torch.tensor([0.05], device=DEV)
    Y = torch.full((B, ncols), 3.0, device=DEV)
    lib().dx_voc_post_c(X.data_ptr(), N * C, W.data_ptr(), bias.data_ptr(), Y.data_ptr(), ncols, fr.data_ptr(), 4, B, N, ncols, C, _stream())
    for b in range(B):
        n = frames[b] * 4
        ref = torch.tanh(F.conv1d(F.leaky_relu(X[b, :n].double(), 0.1).T[None], W.double(), bias.double(), padding=3))[0, 0]
        assert (Y[b, :n].double() - ref).abs().max().item() <= 1e-5
        assert torch.count_nonzero(Y[b, n:]).item() == 0


V3_DILATIONS = {3: (1, 2), 5: (2, 6), 7: (3, 12)}


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C,k', sorted({(c, k) for _, c, k in voc.CHAIN_SHAPES}))
def test_chain_kernel_against_the_two_conv_path_and_torch(C, k, bf16):
    """One ResBlock2 through dx_voc_chain and through two dx_voc_conv calls on the same tensors, for the shapes whose launch path (under
    bf16) is the fused kernel, in both operand modes of the kernel.  f32: <= 1e-6 max (the sums are
    grouped the same per output; the paths differ in where the intermediate is kept).  Both modes: against F.conv1d in float64 on
    operands rounded as the kernels round them."""
    d1, d2 = V3_DILATIONS[k]
    g = torch.Generator().manual_seed(C * 7 + k)
    B, N, scale = 3, 200, 4
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W1 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    W2 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    b1, b2 = (0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    P1, P2 = _pack(W1, 1, bf16), _pack(W2, 1, bf16)
    for mode in (0, 1, 2):
        Y0 = torch.randn(B, N, C, generator=g).to(DEV)
        Y, Z, mid = Y0.clone(), Y0.clone(), torch.empty_like(Y0)
        lib().dx_voc_chain(X.data_ptr(), N * C, P1.data_ptr(), b1.data_ptr(), P2.data_ptr(), b2.data_ptr(), Y.data_ptr(),
                           fr.data_ptr(), scale, B, N, C, k, d1, d2, mode, bf16, _stream())
        lib().dx_voc_conv(X.data_ptr(), N * C, C, 1, P1.data_ptr(), b1.data_ptr(), mid.data_ptr(), N * C, X.data_ptr(),
                          fr.data_ptr(), scale, B, N, C, C, k, d1, 1, 1, 0, bf16, _stream())
        lib().dx_voc_conv(mid.data_ptr(), N * C, C, 1, P2.data_ptr(), b2.data_ptr(), Z.data_ptr(), N * C, mid.data_ptr(),
                          fr.data_ptr(), scale, B, N, C, C, k, d2, 1, 1, mode, bf16, _stream())
        diff = (Y - Z).abs().max().item()
        print(f'chain vs two convs, C {C} k {k} d ({d1}, {d2}) mode {mode} bf16 {bf16}: max abs {diff:.2e}')
        if not bf16:
            assert diff <= 1e-6, (mode, diff)
        for b in range(B):
            n = frames[b] * scale
            x = X[b, :n].double()
            x1 = F.conv1d(_q(F.leaky_relu(x, 0.1), bf16).T[None], _q(W1, bf16), b1.double(), padding=d1 * (k - 1) // 2, dilation=d1)[0].T + x
            ref = F.conv1d(_q(F.leaky_relu(x1, 0.1), bf16).T[None], _q(W2, bf16), b2.double(), padding=d2 * (k - 1) // 2, dilation=d2)[0].T + x1
            ref = _finish(ref, Y0[b, :n].double(), mode)
            assert (Y[b, :n].double() - ref).abs().max().item() <= _tol(ref, bf16), (b, mode)
            assert torch.count_nonzero(Y[b, n:]).item() == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_speech_synthesizer_with_a_v3_vocoder(vocoders):
    import ubisoft_laforge_daft_exprt_amd as dx
    case = helpers.load_case('inference_add')
    hp = helpers.golden_hparams(stats={'spk 0': {'energy': {'mean': 2.0, 'std': 1.5}, 'pitch': {'mean': 5.0, 'std': 0.25}},
                                       'spk 1': {'energy': {'mean': 1.7, 'std': 1.1}, 'pitch': {'mean': 4.6, 'std': 0.3}}})
    dx.set_precision('f32')
    model = dx.DaftExprt(hp).to(DEV)
    model.load_state_dict(helpers.golden_state_dict(), strict=True)
    vocoder = vocoders['v3', 'f32']
    synth = dx.SpeechSynthesizer(model.eval(), hp, vocoder)

    def args():
        t = lambda k: torch.from_numpy(case[k]).clone().to(DEV)
        inputs = (t('in/symbols'), t('in/dur_factors'), t('in/energy_factors'), t('in/pitch_factors'), t('in/input_lengths'), t('in/speaker_ids'))
        prosody = {k: t('in/prosody_' + k) for k in ('duration_preds', 'durations_int', 'energy_preds', 'pitch_preds')}
        return inputs, 'add', prosody, t('in/spk_embs'), t('in/accent_emb')
    ref = synth(*args())
    audio, slen = vocoder.infer_batch(ref['mel'], ref['output_lengths'])
    assert torch.equal(ref['audio'], audio) and torch.equal(ref['sample_lengths'], slen.to(ref['sample_lengths'].dtype))
    assert audio.abs().max().item() > 0
    for use_graph in (True, False):
        out = synth.stream(*args(), use_graph=use_graph, chunk_frames=8)
        pcm, chunks, valid = zip(*list(out['chunks']))
        pcm, chunks = torch.cat(pcm, dim=1), torch.cat(chunks, dim=1)
        cols = min(chunks.shape[1], audio.shape[1])
        assert torch.equal(chunks[:, :cols], audio[:, :cols]) and torch.count_nonzero(chunks[:, cols:]).item() == 0, use_graph
        assert torch.equal(pcm[:, :cols], ref['pcm'][:, :cols])
        assert torch.equal(torch.stack(valid).sum(dim=0), ref['sample_lengths'])
