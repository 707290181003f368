"""HiFi-GAN vocoder throughput (V1, or V2 / V3 with --config): B = 16 synthetic utterances of up to 850 frames (C4-like lengths), synthetic weights.
One JSON line: mel frames/s, seconds of 22.05 kHz audio per second and TFLOP/s against 614 MFLOP per frame, for the HIP path (f32, bf16,
bf16x3), tests/vocoder_torch.py batched on the same GPU (fp32, bf16) and vocoder_torch at B = 1 per utterance (fp32: the reference's way; bf16).
Every rate divides VALID frames by the time.  The HIP path computes valid frames only (tiles past a row's length write zeros); the batched
torch rows compute the whole padded (B, 80, T_max) grid ('frames_computed'), the B = 1 rows exactly the valid frames, so
'hip_bf16_over_torch_bf16_b1' compares equal work and 'hip_bf16_over_torch_bf16' what a caller with a padded batch gets.

    python tools/bench_vocoder.py [--config v1|v2|v3] [--profile] [--hip-only] [--rounds N]

--rounds N: + 'rounds': the three HIP modes timed alternately (f32, bf16x3, bf16; N rounds after one untimed round), per mode the
times of every round, their median and spread (max - min), the ratio of the f32 to the bf16x3 median, and for the bf16x3 mode what
``stream`` takes at 32 frames a chunk: the first chunk's latency (median of 3) and the workspace against ``infer_batch``'s.
--profile: + per-kernel times of one HIP call in each mode; --hip-only: without the torch rows (whose first calls spend minutes in
MIOpen's search over the 16 utterance lengths).

--config v2 / v3: the same batch through the V2 / V3 generator (the same torch rows), FLOP per frame
counted from the configuration's own (unpadded) layer shapes; the default, v1, prints what it always printed.
"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tests import vocoder_helpers as vh  # noqa: E402
from tests import vocoder_torch  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import profiling, vocoder as voc  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import _lib  # noqa: E402

MFLOP_PER_FRAME = 614.0
B, T_MAX = 16, 850


def mflop_per_frame(cfg):
    """2 x taps x Cin x Cout per output sample of every layer of the generator, per mel frame (V1: 614)"""
    c, scale = cfg['upsample_initial_channel'], 1
    flop = 2.0 * 7 * cfg['model_in_dim'] * c
    for u, k, width in zip(cfg['upsample_rates'], cfg['upsample_kernel_sizes'], voc.stage_widths(cfg, padded=False)):
        flop += 2.0 * k * c * width * scale                       # every input row meets all k taps of the transposed conv
        c, scale = width, scale * u
        for kk, ds in zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes']):
            flop += 2.0 * kk * c * c * scale * len(ds) * (1 if str(cfg['resblock']) == '2' else 2)
    return round((flop + 2.0 * 7 * c * scale) / 1e6, 1)


def timed(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def rates(t, frames, computed=None):
    """valid-frame rates; ``computed``: frames the path actually computes (padding included), reported with its own TFLOP/s."""
    r = {'s': round(t, 5), 'frames_per_s': round(frames / t, 1), 'audio_s_per_s': round(frames * 256 / 22050 / t, 1),
         'tflops': round(frames * MFLOP_PER_FRAME * 1e6 / t / 1e12, 2)}
    if computed is not None:
        r.update(frames_computed=computed, tflops_computed=round(computed * MFLOP_PER_FRAME * 1e6 / t / 1e12, 2))
    return r


def alternated(voc_by, mels, lens_dev, frames, n_rounds):
    """The modes in turn, round after round, so that a drift of the clocks meets all of them alike."""
    order = ('f32', 'bf16x3', 'bf16')
    times = {p: [] for p in order}
    for r in range(n_rounds + 1):                                     # round 0 warms every mode up and is not kept
        for p in order:
            t = timed(lambda: voc_by[p].infer_batch(mels, lens_dev), n=8, warm=1)
            if r:
                times[p].append(t)
    out = {p: {'s': [round(t, 5) for t in ts], 'median_s': round(statistics.median(ts), 5), 'spread_s': round(max(ts) - min(ts), 5),
               'tflops': round(frames * MFLOP_PER_FRAME * 1e6 / statistics.median(ts) / 1e12, 2)} for p, ts in times.items()}
    out['f32_over_bf16x3'] = round(out['f32']['median_s'] / out['bf16x3']['median_s'], 3)
    out['bf16x3_over_bf16'] = round(out['bf16x3']['median_s'] / out['bf16']['median_s'], 3)
    out['bf16x3_faster_than_f32_by_more_than_the_spread'] = bool(
        min(times['f32']) - max(times['bf16x3']) > max(out[p]['spread_s'] for p in order))
    return out


def stream_record(v, mels, lens_dev, F=32):
    """first-chunk latency of ``stream`` (from its call to a synchronise after chunk 0; median of 3 after one warm-up) and workspace"""
    def first():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = v.stream(mels, lens_dev, chunk_frames=F, clone=False)
        next(s)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, s
    first()
    runs = [first() for _ in range(3)]
    return {'chunk_frames': F, 'first_chunk_ms': round(statistics.median(t for t, _ in runs) * 1e3, 3),
            'workspace': {'stream': runs[0][1].workspace_bytes, 'stream_rings_per_row': runs[0][1].plan.ring_bytes(1),
                          'infer_batch': B * T_MAX * voc.workspace_bytes_per_frame(v.config)}}


def main():
    global MFLOP_PER_FRAME
    dev = 'cuda'
    name = sys.argv[sys.argv.index('--config') + 1] if '--config' in sys.argv else 'v1'
    if name not in voc.CONFIGS:
        raise SystemExit(f'--config takes one of {sorted(voc.CONFIGS)}, got {name!r}')
    cfg = voc.CONFIGS[name]()
    torch_generator = lambda m, w: vocoder_torch.generator(m, w, cfg)
    if name != 'v1':
        MFLOP_PER_FRAME = mflop_per_frame(cfg)
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(T_MAX // 2, T_MAX + 1, (B,), generator=g)
    lengths[0] = T_MAX
    frames = int(lengths.sum())
    mels = ((torch.randn(B, 80, T_MAX, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0)).to(dev)
    for b, n in enumerate(lengths.tolist()):
        mels[b, :, n:] = 0
    lens_dev = lengths.to(dev)
    sd = vh.state_dict(name)
    out = {'workload': f'B={B} utterances, {frames} mel frames (max {T_MAX})', 'mflop_per_frame': MFLOP_PER_FRAME}
    if name != 'v1':
        out['config'] = name
    voc_by = {}
    with torch.no_grad():
        for prec in ('f32', 'bf16', 'bf16x3'):
            v = voc.HiFiGanVocoder(sd, config=cfg, device=dev, precision=prec)
            voc_by[prec] = v
            out[f'hip_{prec}'] = rates(timed(lambda: v.infer_batch(mels, lens_dev)), frames)
        if '--hip-only' not in sys.argv:
            w32 = vocoder_torch.to(voc_by['f32'].weights, dev)
            w16 = vocoder_torch.to(voc_by['f32'].weights, dev, torch.bfloat16)
            padded = B * T_MAX
            out['torch_fp32_batched'] = rates(timed(lambda: torch_generator(mels, w32)), frames, padded)
            m16 = mels.to(torch.bfloat16)
            out['torch_bf16_batched'] = rates(timed(lambda: torch_generator(m16, w16)), frames, padded)
            per = [mels[b:b + 1, :, :n].contiguous() for b, n in enumerate(lengths.tolist())]
            out['torch_fp32_b1'] = rates(timed(lambda: [torch_generator(m, w32) for m in per], n=2, warm=1), frames, frames)
            per16 = [m.to(torch.bfloat16) for m in per]
            out['torch_bf16_b1'] = rates(timed(lambda: [torch_generator(m, w16) for m in per16], n=2, warm=1), frames, frames)
            out['hip_bf16_over_torch_bf16'] = round(out['torch_bf16_batched']['s'] / out['hip_bf16']['s'], 2)
            out['hip_bf16_over_torch_bf16_b1'] = round(out['torch_bf16_b1']['s'] / out['hip_bf16']['s'], 2)
        if '--rounds' in sys.argv:
            out['rounds'] = alternated(voc_by, mels, lens_dev, frames, int(sys.argv[sys.argv.index('--rounds') + 1]))
            out['stream_bf16x3'] = stream_record(voc_by['bf16x3'], mels, lens_dev)
        if '--profile' in sys.argv:
            geom = profiling.Geometry([lengths.tolist()])
            for prec in ('bf16', 'f32', 'bf16x3'):
                recs = []
                old = _lib.set_timer(recs)
                voc_by[prec].infer_batch(mels, lens_dev)
                _lib.set_timer(old)
                torch.cuda.synchronize()
                out[f'profile_{prec}'] = profiling.summarize(recs, geom, prec)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
