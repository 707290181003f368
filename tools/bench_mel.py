"""Mel front end throughput on the vocoder bench's lengths: B = 16 utterances, 10 644 valid frames, longest 850 (tools/bench_vocoder.py),
as waveforms of 256 frames + 128 samples each.  One JSON line: ms, frames/s, seconds of 22.05 kHz audio per second and TFLOP/s for
  hip              MelSpectrogram (csrc/dx_mel.hip), one launch for the batch, host lengths
  torch_gpu_b1     the reference's way on the same GPU: torch reflect pad + stft + matmul + log + energy, B = 1 per utterance
  torch_gpu_padded torch on the padded (B, S_max) batch (timing only: its row ends differ from the per-utterance result)
  torch_cpu_b1     the reference as it runs: the same torch code on the CPU, per utterance
TFLOP/s counts the direct-DFT work of valid frames (2 * 1024 * 2 * 372 + 2 * 372 * 80 FLOP per frame); 'hip' adds the rate on the
work it executes (whole 32-frame tiles, 384 bins).  'hip_over_vocoder_bf16' is the HIP time over one bf16 HiFiGanVocoder.infer_batch
call on the resulting mels (the issue's budget: 2 %).  GPU times are event-bracketed means after warm-up.

    python tools/bench_mel.py
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from ubisoft_laforge_daft_exprt_amd import mel  # noqa: E402

B, T_MAX = 16, 850
KMAX, KMAXP, NMEL = 372, 384, 80
FLOP_PER_FRAME = 2.0 * 1024 * 2 * KMAX + 2.0 * KMAX * NMEL


def gpu_time(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def cpu_time(fn, n=2, warm=1):
    for _ in range(warm):
        fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n


def rates(t, frames, executed_flop=None):
    r = {'ms': round(t * 1e3, 4), 'frames_per_s': round(frames / t, 1), 'audio_s_per_s': round(frames * 256 / 22050 / t, 1),
         'tflops': round(frames * FLOP_PER_FRAME / t / 1e12, 2)}
    if executed_flop is not None:
        r['tflops_executed'] = round(executed_flop / t / 1e12, 2)
    return r


def torch_mel(y, fb, window):
    """(B, S) -> (log-mel, energy): the reference's mel_spectrogram_HiFi + extract_energy(np.exp(mel)) in torch."""
    y = torch.nn.functional.pad(y[:, None], (384, 384), mode='reflect')[:, 0]
    spec = torch.stft(y, 1024, hop_length=256, win_length=1024, window=window, center=False, return_complex=True)
    spec = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    m = torch.log(torch.clamp(torch.matmul(fb, spec), min=1e-5))
    return m, torch.linalg.vector_norm(torch.exp(m), dim=1)


def main():
    dev = 'cuda'
    g = torch.Generator().manual_seed(3)
    frames_b = torch.randint(T_MAX // 2, T_MAX + 1, (B,), generator=g)
    frames_b[0] = T_MAX
    lens = [int(f) * 256 + 128 for f in frames_b]
    frames = sum(n // 256 for n in lens)
    S = max(lens)
    wavs = torch.zeros(B, S)
    for b, n in enumerate(lens):
        wavs[b, :n] = 0.3 * torch.randn(n, generator=g)
    wavs = wavs.to(dev)
    fe = mel.MelSpectrogram(device=dev)
    out = {'workload': f'B={B} utterances, {frames} valid mel frames (max {T_MAX}), {sum(lens)} samples',
           'flop_per_frame': FLOP_PER_FRAME}
    executed = sum((n // 256 + 31) // 32 * 32 for n in lens) * (2.0 * 1024 * 2 * KMAXP + 2.0 * KMAXP * NMEL)
    with torch.no_grad():
        t_hip = gpu_time(lambda: fe(wavs, lens))
        out['hip'] = rates(t_hip, frames, executed)
        fb = torch.from_numpy(fe.filter_bank).to(dev)
        win = torch.hann_window(1024, device=dev)
        per = [wavs[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
        out['torch_gpu_b1'] = rates(gpu_time(lambda: [torch_mel(y, fb, win) for y in per], n=5), frames)
        out['torch_gpu_padded'] = rates(gpu_time(lambda: torch_mel(wavs, fb, win), n=10), frames)
        fbc, winc = fb.cpu(), torch.hann_window(1024)
        perc = [y.cpu() for y in per]
        out['torch_cpu_b1'] = rates(cpu_time(lambda: [torch_mel(y, fbc, winc) for y in perc]), frames)
        out['torch_cpu_threads'] = torch.get_num_threads()
        out['hip_over_torch_gpu_b1'] = round(out['torch_gpu_b1']['ms'] / out['hip']['ms'], 2)
        out['hip_over_torch_gpu_padded'] = round(out['torch_gpu_padded']['ms'] / out['hip']['ms'], 2)
        out['hip_over_torch_cpu_b1'] = round(out['torch_cpu_b1']['ms'] / out['hip']['ms'], 1)
        # parity of the timed HIP output against the per-utterance torch path (fp32 both), for the record
        mels, energy, _ = fe(wavs, lens)
        err = max(float((mels[b, :, :n // 256] - torch_mel(y, fb, win)[0][0]).abs().max()) for b, (n, y) in enumerate(zip(lens, per)))
        out['hip_vs_torch_b1_max_abs_logmel'] = err
        if '--no-vocoder' not in sys.argv:
            from tests import vocoder_helpers as vh
            from ubisoft_laforge_daft_exprt_amd import vocoder as voc
            v = voc.HiFiGanVocoder(vh.state_dict(), device=dev, precision='bf16')
            fr = torch.tensor([n // 256 for n in lens], device=dev)
            t_voc = gpu_time(lambda: v.infer_batch(mels, fr), n=3, warm=1)
            out['vocoder_bf16_infer_batch_ms'] = round(t_voc * 1e3, 3)
            out['hip_over_vocoder_bf16'] = round(t_hip / t_voc, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
