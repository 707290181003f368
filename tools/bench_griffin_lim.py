"""Griffin-Lim on the device at the vocoder bench's lengths: B = 1 at 850 frames and B = 16 utterances with 10 644 valid mel frames
(longest 850; the lengths of tools/bench_mel.py).  One JSON line with, for each workload,
  gl_iter_us       microseconds per Griffin-Lim iteration: a ``reconstruct`` call of 500 iterations over 500, eager (500 launches
                   enqueued by the host) and graph (one replay of the captured chain, plus the copies into its buffers and the clone out)
  nnls_ms          ``mel_to_linear`` (200 FISTA steps)
  from_mel_ms      the whole ``from_mel`` (exp, NNLS, 500 iterations, peak normalisation), eager and graph
Times are device events around repeated calls after a warm-up of every shape (the warm-up also captures the graphs).  'reference_cpu'
repeats the figures measured for the reference on CPU in float64 (one 129-frame utterance: 2.4 s in mel_to_linear, 8.3 ms per
Griffin-Lim iteration, both growing with the length), for the same page; they are not re-measured here.

    python tools/bench_griffin_lim.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from ubisoft_laforge_daft_exprt_amd import griffin_lim as gl  # noqa: E402

B, T_MAX, ITERS = 16, 850, 500


def gpu_time(fn, n=5, warm=2):
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


def workload(engine, mels, lens):
    frames = sum(lens)
    Bn, _, T = mels.shape
    out = {'B': Bn, 'valid_frames': frames, 'T_max': T}
    X = engine.mel_to_linear(torch.exp(mels), lens)
    glens = [max(n - 2, 0) for n in lens]
    init = torch.randn(Bn, 256 * (T - 2) + 1024, device=mels.device)
    for mode, use_graph in (('eager', False), ('graph', True)):
        t = gpu_time(lambda: engine.reconstruct(X[:, :, :T - 2], glens, init=init, iterations=ITERS, use_graph=use_graph))
        out[f'gl_iter_us_{mode}'] = round(t / ITERS * 1e6, 2)
        t = gpu_time(lambda: engine.from_mel(mels, lens, init=init, iterations=ITERS, use_graph=use_graph))
        out[f'from_mel_ms_{mode}'] = round(t * 1e3, 3)
    out['nnls_ms'] = round(gpu_time(lambda: engine.mel_to_linear(torch.exp(mels), lens), n=10) * 1e3, 3)
    out['audio_s'] = round(sum(256 * n + 512 for n in lens) / 22050, 2)
    return out


def main():
    if not torch.cuda.is_available():
        raise RuntimeError('bench_griffin_lim needs a GPU')
    dev = 'cuda'
    g = torch.Generator().manual_seed(3)
    frames_b = torch.randint(T_MAX // 2, T_MAX + 1, (B,), generator=g)
    frames_b[0] = T_MAX
    lens = [int(f) for f in frames_b]
    mels = torch.full((B, 80, T_MAX), -11.5)
    for b, n in enumerate(lens):                                   # a smooth speech-like envelope with noise on top, in log-mel range
        t = torch.arange(n)[None, :] / 40.0
        c = torch.arange(80)[:, None] / 80.0
        mels[b, :, :n] = -4.0 + 2.5 * torch.sin(t + 6.0 * c) - 3.0 * c + 0.5 * torch.randn(80, n, generator=g)
    mels = mels.to(dev)
    engine = gl.GriffinLim(device=dev)
    out = {'iterations': ITERS, 'nnls_iterations': engine.nnls_iterations}
    with torch.no_grad():
        out['b1'] = workload(engine, mels[:1].contiguous(), lens[:1])
        out['b16'] = workload(engine, mels, lens)
    out['reference_cpu'] = {'frames': 129, 'mel_to_linear_s': 2.4, 'gl_iter_ms': 8.3, 'gl_500_iterations_s': 4.1, 'note': 'float64, one utterance; grows with length'}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
