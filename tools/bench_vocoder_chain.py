"""One V3 ResBlock2 as the fused dx_voc_chain launch against the same block as two dx_voc_conv launches, at the rows the stage has in
tools/bench_vocoder.py's batch (B = 16 utterances of 425 .. 850 frames; 64 samples per frame at 64 channels, 256 at 32), in both
operand modes.  One JSON line: ms per block for each form (device events around 20 launches after 3 warm-ups) and the largest
difference between the two results.  vocoder.CHAIN_SHAPES lists the shapes for which the fused form is the launch path.

    python tools/bench_vocoder_chain.py
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tools.bench_vocoder import B, T_MAX  # noqa: E402
from ubisoft_laforge_daft_exprt_amd._lib import lib, packed as _packed  # noqa: E402

DILATIONS = {3: (1, 2), 5: (2, 6), 7: (3, 12)}
SCALE = {64: 64, 32: 256}


def timed_ms(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


def main():
    dev = torch.device('cuda')
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(T_MAX // 2, T_MAX + 1, (B,), generator=g)
    lengths[0] = T_MAX
    fr = lengths.to(device=dev, dtype=torch.int32)
    out = {'workload': f'B={B} utterances, {int(lengths.sum())} mel frames (max {T_MAX})'}
    L = lib()
    for C, scale in SCALE.items():
        N = T_MAX * scale
        X = torch.randn(B, N, C, generator=g).to(dev)
        Y, Z, mid = torch.zeros_like(X), torch.zeros_like(X), torch.zeros_like(X)
        for k, (d1, d2) in DILATIONS.items():
            W = [(torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).to(dev) for _ in range(2)]
            b1, b2 = (0.1 * torch.randn(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
            for bf16, prec in ((0, 'f32'), (1, 'bf16')):
                P1, P2 = (_packed('voc', w, (C, C, k, 1, bf16), dev) for w in W)

                def chain():
                    L.dx_voc_chain(X.data_ptr(), N * C, P1.data_ptr(), b1.data_ptr(), P2.data_ptr(), b2.data_ptr(), Y.data_ptr(),
                                   fr.data_ptr(), scale, B, N, C, k, d1, d2, 0, bf16, st)

                def two():
                    L.dx_voc_conv(X.data_ptr(), N * C, C, 1, P1.data_ptr(), b1.data_ptr(), mid.data_ptr(), N * C, X.data_ptr(),
                                  fr.data_ptr(), scale, B, N, C, C, k, d1, 1, 1, 0, bf16, st)
                    L.dx_voc_conv(mid.data_ptr(), N * C, C, 1, P2.data_ptr(), b2.data_ptr(), Z.data_ptr(), N * C, mid.data_ptr(),
                                  fr.data_ptr(), scale, B, N, C, C, k, d2, 1, 1, 0, bf16, st)
                a, b = timed_ms(chain), timed_ms(two)
                a2, b2_ = timed_ms(chain), timed_ms(two)                  # alternated: the spread of a repeat, not one sample
                out[f'C{C}_k{k}_d{d1}_{d2}_{prec}'] = {'chain_ms': [round(a, 4), round(a2, 4)], 'two_convs_ms': [round(b, 4), round(b2_, 4)],
                                                      'max_abs_diff': float((Y - Z).abs().max())}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
