"""The gfx950 HiFi-GAN vocoder on the GPU: parity with the reference golden (f32), bf16 against f32, batch rows bitwise equal to the
utterance run alone, chunking, per-kernel checks against F.conv1d / F.conv_transpose1d, and the synthesizer -> vocoder path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helpers
from tests import vocoder_helpers as vh
from tests import vocoder_torch
from ubisoft_laforge_daft_exprt_amd import vocoder as voc
from ubisoft_laforge_daft_exprt_amd._lib import lib

DEV = 'cuda:0'
pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope='module')
def vocoders():
    sd = vh.state_dict()
    return {p: voc.HiFiGanVocoder(sd, device=DEV, precision=p) for p in ('f32', 'bf16')}


def test_f32_matches_reference_golden(vocoders):
    lengths, mels, wavs = vh.golden()
    for n, mel, ref in zip(lengths, mels, wavs):
        got = vocoders['f32'].infer(mel)
        err = np.abs(got - ref)
        print(f'f32 vs reference, {n} frames: max {err.max():.2e} mean {err.mean():.2e}')
        assert got.shape == ref.shape
        assert err.max() <= 1e-5 and err.mean() <= 1e-6, (n, err.max(), err.mean())


def test_bf16_against_f32_snr(vocoders):
    lengths, mels, _ = vh.golden()
    for n, mel in zip(lengths, mels):
        a = vocoders['f32'].infer(mel).astype(np.float64)
        b = vocoders['bf16'].infer(mel).astype(np.float64)
        snr = 10 * np.log10((a ** 2).sum() / max(((a - b) ** 2).sum(), 1e-30))
        print(f'bf16 vs f32, {n} frames: SNR {snr:.1f} dB')
        assert snr >= 35.0, (n, snr)


# 1 frame: every halo is larger than the utterance; 3, 4, 5, 8, 9 frames straddle the 64-sample tiles of stage 0 (8, 32 samples per
# frame...) and stage 1 onwards; 40 / 41 cross several tiles at every stage
BATCH_LENGTHS = [1, 41, 3, 8, 9, 4, 5, 40, 17]


def _batch():
    g = torch.Generator().manual_seed(5)
    T = max(BATCH_LENGTHS)
    mels = (torch.randn(len(BATCH_LENGTHS), 80, T, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0)
    return mels.to(DEV)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_batch_rows_equal_utterances_alone_bitwise(vocoders, precision):
    v = vocoders[precision]
    mels = _batch()
    audio, slen = v.infer_batch(mels, BATCH_LENGTHS)
    assert audio.shape == (len(BATCH_LENGTHS), 256 * mels.shape[2]) and slen == [256 * n for n in BATCH_LENGTHS]
    for b, n in enumerate(BATCH_LENGTHS):
        alone, _ = v.infer_batch(mels[b:b + 1, :, :n].contiguous(), [n])
        assert torch.equal(audio[b, :256 * n], alone[0]), (precision, b, n)
        assert torch.count_nonzero(audio[b, 256 * n:]).item() == 0
        assert torch.count_nonzero(alone[0]).item() > 0
    # lengths as the device tensor GraphedSynthesizer returns: same result, device sample lengths
    audio2, slen2 = v.infer_batch(mels, torch.tensor(BATCH_LENGTHS, device=DEV))
    assert torch.equal(audio, audio2) and torch.equal(slen2.cpu(), torch.tensor(BATCH_LENGTHS) * 256)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_chunking_under_workspace_bound_is_bitwise_neutral(vocoders, precision):
    v = vocoders[precision]
    mels = _batch()
    whole, _ = v.infer_batch(mels, BATCH_LENGTHS)
    bound = 2 * 41 * voc.WORKSPACE_BYTES_PER_FRAME
    chunked, _ = v.infer_batch(mels, BATCH_LENGTHS, max_workspace_bytes=bound)
    assert torch.equal(whole, chunked)


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
    return (2e-2 if bf16 else 2e-5) * max(1.0, ref.abs().max().item())


def _lens(B, N, scale):
    frames = [max(1, (N // scale) - 3 * b) for b in range(B)]
    return frames, torch.tensor(frames, dtype=torch.int32, device=DEV)


CONV_SHAPES = [(C, k, d) for C in (256, 128, 64, 32) for k in (3, 7, 11) for d in (1, 3, 5)]


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C,k,d', CONV_SHAPES)
def test_dilated_conv_kernel(C, k, d, bf16):
    g = torch.Generator().manual_seed(C * 100 + k * 10 + d)
    B, N, scale = 3, 150, 2
    frames, fr = _lens(B, N, scale)
    X = torch.randn(B, N, C, generator=g).to(DEV)
    W = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(C, generator=g)).to(DEV)
    Wp = _pack(W, 1, bf16)
    for mode, resid in ((0, False), (0, True), (1, True), (2, True)):
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
            if mode == 1:
                ref = Y0[b, :n].double() + ref
            elif mode == 2:
                ref = (Y0[b, :n].double() + ref) / 3
            assert (Y[b, :n].double() - ref).abs().max().item() <= _tol(ref, bf16), (b, mode)
            assert torch.count_nonzero(Y[b, n:]).item() == 0


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C,k,d', [(C, k, d) for C in (64, 32) for k in (3, 7, 11) for d in (1, 3, 5)])
def test_fused_pair_kernel(C, k, d, bf16):
    g = torch.Generator().manual_seed(C * 7 + k * 3 + d)
    B, N, scale = 3, 200, 4
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
            if mode == 1:
                ref = Y0[b, :n].double() + ref
            elif mode == 2:
                ref = (Y0[b, :n].double() + ref) / 3
            assert (Y[b, :n].double() - ref).abs().max().item() <= _tol(ref, bf16), (b, mode)
            assert torch.count_nonzero(Y[b, n:]).item() == 0


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('Cin,u', [(512, 8), (256, 8), (128, 2), (64, 2)])
def test_transposed_conv_kernel(Cin, u, bf16):
    g = torch.Generator().manual_seed(Cin + u)
    Cout, B, N, scale = Cin // 2, 3, 70, 1
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
        assert ref.shape[0] == n * u
        assert (Y[b, :n * u].double() - ref).abs().max().item() <= _tol(ref, bf16), b
        assert torch.count_nonzero(Y[b, n * u:]).item() == 0


@pytest.mark.parametrize('bf16', [0, 1])
def test_conv_pre_reads_the_mel_layout(bf16):
    g = torch.Generator().manual_seed(11)
    B, T, N = 3, 90, 77                                          # N < T: the work is sized to the longest row, not the padding
    frames, fr = [77, 1, 50], torch.tensor([77, 1, 50], dtype=torch.int32, device=DEV)
    mel = torch.randn(B, 80, T, generator=g).to(DEV)
    W = (torch.randn(512, 80, 7, generator=g) / (80 * 7) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(512, generator=g)).to(DEV)
    Wp = _pack(W, 1, bf16)
    Y = torch.empty(B, N, 512, device=DEV)
    lib().dx_voc_conv(mel.data_ptr(), 80 * T, 1, T, Wp.data_ptr(), bias.data_ptr(), Y.data_ptr(), N * 512, None,
                      fr.data_ptr(), 1, B, N, 80, 512, 7, 1, 1, 0, 0, bf16, _stream())
    for b in range(B):
        n = frames[b]
        ref = F.conv1d(_q(mel[b:b + 1, :, :n], bf16), _q(W, bf16), bias.double(), padding=3)[0].T
        assert (Y[b, :n].double() - ref).abs().max().item() <= _tol(ref, bf16), b
        assert torch.count_nonzero(Y[b, n:]).item() == 0


def test_conv_post_kernel():
    g = torch.Generator().manual_seed(12)
    B, N, ncols = 2, 300, 320
    frames, fr = [300 // 4, 20], torch.tensor([300 // 4, 20], dtype=torch.int32, device=DEV)
    X = torch.randn(B, N, 32, generator=g).to(DEV)
    W = (torch.randn(1, 32, 7, generator=g) / 8).to(DEV)
    bias = torch.tensor([0.05], device=DEV)
    Y = torch.full((B, ncols), 3.0, device=DEV)
    lib().dx_voc_post(X.data_ptr(), N * 32, W.data_ptr(), bias.data_ptr(), Y.data_ptr(), ncols, fr.data_ptr(), 4, B, N, ncols, _stream())
    for b in range(B):
        n = frames[b] * 4
        ref = torch.tanh(F.conv1d(F.leaky_relu(X[b, :n].double(), 0.1).T[None], W.double(), bias.double(), padding=3))[0, 0]
        assert (Y[b, :n].double() - ref).abs().max().item() <= 1e-5
        assert torch.count_nonzero(Y[b, n:]).item() == 0


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_synthesizer_batch_to_audio_in_one_call(vocoders):
    import ubisoft_laforge_daft_exprt_amd as dx
    from ubisoft_laforge_daft_exprt_amd.inference import GraphedSynthesizer
    case = helpers.load_case('inference_add')
    hp = helpers.golden_hparams(stats={'spk 0': {'pitch': {'mean': 5.0, 'std': 0.25}}, 'spk 1': {'pitch': {'mean': 4.6, 'std': 0.3}}})
    dx.set_precision('f32')
    model = dx.DaftExprt(hp).to(DEV)
    model.load_state_dict(helpers.golden_state_dict(), strict=True)
    synth = GraphedSynthesizer(model.eval(), hp)
    t = lambda k: torch.from_numpy(case[k]).clone().to(DEV)
    inputs = (t('in/symbols'), t('in/dur_factors'), t('in/energy_factors'), t('in/pitch_factors'), t('in/input_lengths'), t('in/speaker_ids'))
    prosody = {k: t('in/prosody_' + k) for k in ('duration_preds', 'durations_int', 'energy_preds', 'pitch_preds')}
    _, (mel, out_lens), _ = synth(inputs, 'add', prosody, t('in/spk_embs'), t('in/accent_emb'), use_graph=True)
    audio, slen = vocoders['f32'].infer_batch(mel, out_lens)
    weights = vocoder_torch.to(vocoders['f32'].weights, DEV)
    for b, n in enumerate(out_lens.tolist()):
        with torch.no_grad():
            ref = vocoder_torch.generator(mel[b:b + 1, :, :n].float(), weights)[0]
        err = (audio[b, :256 * n] - ref).abs().max().item()
        print(f'synthesizer row {b} ({n} frames): max abs vs torch {err:.2e}')
        assert err <= 1e-4, (b, err)
        assert int(slen[b]) == 256 * n and torch.count_nonzero(audio[b, 256 * n:]).item() == 0
