"""Forward + backward of the mel L1 loss (mel.MelL1Loss, csrc/dx_mel.hip dx_mel + dx_mel_bwd) on two shapes:
  vocoder_batch   B = 16 utterances, 10 644 valid frames, longest 850 (the lengths of tools/bench_mel.py and tools/bench_vocoder.py)
  finetune        B = 16 segments of 8192 samples, 32 frames each (the reference's vocoder fine-tuning segment)
One JSON line per shape: ms of
  hip_fwd_bwd       loss = MelL1Loss(wav, lengths, target); loss.backward()      (full-band mel, as the reference's loss)
  hip_fwd           the forward launch alone (MelSpectrogram under no_grad)
  hip_bwd_launch    dx_mel_bwd alone (an upstream gradient of ones)
  torch_b1          torch autograd of the same function on the same GPU, B = 1 per utterance (the reference's way)
  torch_padded      torch autograd on the padded (B, S_max) batch (its row ends differ from the per-utterance result: timing only)
and the largest |gradient difference| of the HIP path against torch_b1, relative to the largest gradient.  GPU times are
event-bracketed means over a window of at least 0.3 s after warm-up; each figure is taken three times, alternating the paths, and the
median is reported with the spread.

    python tools/bench_mel_backward.py
"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from ubisoft_laforge_daft_exprt_amd import mel  # noqa: E402

B, T_MAX, NMEL = 16, 850, 80


def gpu_time(fn, min_s=0.3, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    n, total = 4, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        total = a.elapsed_time(b) / 1e3
        if total >= min_s:
            return total / n
        n = max(n * 2, int(n * min_s / max(total, 1e-6) * 1.2))


def torch_loss(y, lengths, target, fb, window):
    """F.l1_loss(target, mel(y)) * 45 with the reference's mel_spectrogram in torch; lengths only shape the padded batch."""
    yp = torch.nn.functional.pad(y[:, None], (384, 384), mode='reflect')[:, 0]
    spec = torch.stft(yp, 1024, hop_length=256, win_length=1024, window=window, center=False, return_complex=True)
    mag = torch.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    m = torch.log(torch.clamp(torch.matmul(fb, mag), min=1e-5))
    return torch.nn.functional.l1_loss(target[:, :, :m.shape[2]], m) * 45


def shape(name, lens, dev, gen):
    S, T = max(lens), max(lens) // 256
    frames = sum(n // 256 for n in lens)
    wavs = torch.zeros(B, S)
    for b, n in enumerate(lens):
        wavs[b, :n] = 0.3 * torch.randn(n, generator=gen)
    wavs = wavs.to(dev)
    target = (torch.randn(B, NMEL, T, generator=gen) - 5.0).to(dev)
    loss_fn = mel.MelL1Loss(fmax=None, device=dev)
    fe = loss_fn.frontend
    fb = torch.from_numpy(fe.filter_bank).to(dev)
    win = torch.hann_window(1024, device=dev)
    w = wavs.clone().requires_grad_(True)
    per = [wavs[b:b + 1, :n].clone().requires_grad_(True) for b, n in enumerate(lens)]
    per_t = [target[b:b + 1, :, :n // 256].contiguous() for b, n in enumerate(lens)]
    ones = torch.ones(B, NMEL, T, device=dev)
    lens_i32 = torch.tensor(lens, dtype=torch.int32, device=dev)

    def hip_fwd_bwd():
        w.grad = None
        loss_fn(w, lens, target).backward()

    def hip_fwd():
        with torch.no_grad():
            fe(wavs, lens)

    def hip_bwd_launch():
        fe._launch_backward(wavs, lens_i32, ones)

    def torch_b1():
        for y, t in zip(per, per_t):
            y.grad = None
            torch_loss(y, None, t, fb, win).backward()

    def torch_padded():
        w.grad = None
        torch_loss(w, lens, target, fb, win).backward()

    paths = dict(hip_fwd_bwd=hip_fwd_bwd, hip_fwd=hip_fwd, hip_bwd_launch=hip_bwd_launch, torch_b1=torch_b1, torch_padded=torch_padded)
    runs = {k: [] for k in paths}
    for _ in range(3):                                   # alternate the paths; report the median and the spread
        for k, fn in paths.items():
            runs[k].append(gpu_time(fn))
    out = {'shape': name, 'workload': f'B={B}, {frames} valid frames (max {T}), {sum(lens)} samples'}
    for k, v in runs.items():
        out[k] = {'ms': round(statistics.median(v) * 1e3, 4), 'min_ms': round(min(v) * 1e3, 4), 'max_ms': round(max(v) * 1e3, 4)}
    ms = lambda k: out[k]['ms']
    out['bwd_launch_over_fwd_launch'] = round(ms('hip_bwd_launch') / ms('hip_fwd'), 2)
    out['torch_b1_over_hip'] = round(ms('torch_b1') / ms('hip_fwd_bwd'), 2)
    out['torch_padded_over_hip'] = round(ms('torch_padded') / ms('hip_fwd_bwd'), 2)
    flop = 2.0 * frames * 2 * (1024 * 2 * fe.kmax + fe.kmax * NMEL)
    out['bwd_tflops'] = round(flop / (ms('hip_bwd_launch') * 1e-3) / 1e12, 1)
    # gradient of the per-row loss 45 * mean over the row's own cells, HIP against torch per utterance, for the record
    err = top = 0.0
    for b, n in enumerate(lens):
        y = wavs[b:b + 1, :n].clone().requires_grad_(True)
        loss_fn(y, [n], per_t[b]).backward()
        per[b].grad = None
        torch_loss(per[b], None, per_t[b], fb, win).backward()
        err = max(err, float((y.grad - per[b].grad).abs().max()))
        top = max(top, float(per[b].grad.abs().max()))
    out['hip_vs_torch_b1_grad_rel_max'] = err / top
    print(json.dumps(out), flush=True)


def main():
    dev = 'cuda'
    gen = torch.Generator().manual_seed(3)
    frames_b = torch.randint(T_MAX // 2, T_MAX + 1, (B,), generator=gen)
    frames_b[0] = T_MAX
    shape('vocoder_batch', [int(f) * 256 + 128 for f in frames_b], dev, gen)
    shape('finetune', [8192] * B, dev, gen)


if __name__ == '__main__':
    main()
