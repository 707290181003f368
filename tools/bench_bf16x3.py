"""The split-bf16 mode against its neighbours: the C2 training step (the bench.py workload, graph-replayed Trainer steps) in f32, bf16x3
and bf16, alternated for three rounds, then the per-kernel table of one eager bf16x3 step (us, fraction of the peak: 833 TF/s
fp32-equivalent for the split kernels) and C4 inference in bf16x3 (tools/bench_inference.py).  One JSON document on stdout.

    python tools/bench_bf16x3.py [--steps 20] [--warmup 3] [--rounds 3] [--no-inference] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ('f32', 'bf16x3', 'bf16')


def make_trainer(prec, dev):
    import ubisoft_laforge_daft_exprt_amd as pkg
    from ubisoft_laforge_daft_exprt_amd.loss import pitch_predictor_shapes
    from ubisoft_laforge_daft_exprt_amd.synth import CONFIGS, synthetic_batch, synthetic_state_dict
    from ubisoft_laforge_daft_exprt_amd.trainer import Trainer
    pkg.set_precision(prec)
    try:
        hp = pkg.HyperParams(n_speakers=2)
        model = pkg.DaftExprt(hp).to(dev)
        model.load_state_dict(synthetic_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1234), strict=True)
        model.train()
        crit = pkg.DaftExprtLoss(dev, hp)
        crit.load_pitch_predictor(synthetic_state_dict(pitch_predictor_shapes(), 1235))
    finally:
        pkg.set_precision('f32')
    cfg = dict(CONFIGS['C2'])
    cfg['n_speakers'] = 2
    batch = synthetic_batch(**cfg)
    dev_batch = tuple(t.to(dev) if torch.is_tensor(t) else t for t in batch)
    for i in (5, 9):
        dev_batch[i]._dx_host_lengths = batch[i].tolist()
    trainer = Trainer(model, crit, hp, use_graphs=True, cuts=0)
    return trainer, trainer.resident_batch(dev_batch), (batch[5].tolist(), batch[9].tolist())


def time_steps(trainer, batch, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        trainer.train_step([batch])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def kernel_table(trainer, batch, lens, prec):
    from ubisoft_laforge_daft_exprt_amd import _lib, profiling
    geom = profiling.Geometry(lens)
    trainer.use_graphs = False
    recs = []
    old = _lib.set_timer(recs)
    try:
        trainer.train_step([batch])
        torch.cuda.synchronize()
    finally:
        _lib.set_timer(old)
        trainer.use_graphs = True
    return profiling.summarize(recs, geom, prec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-inference', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    runs = {p: make_trainer(p, dev) for p in MODES}
    for p, (t, b, _) in runs.items():
        for _ in range(args.warmup):
            t.train_step([b])
    ms = {p: [] for p in MODES}
    for _ in range(args.rounds):
        for p in MODES:
            t, b, _ = runs[p]
            ms[p].append(round(time_steps(t, b, args.steps) * 1e3, 3))
    frames = sum(runs['f32'][2][1])
    out = {'c2_ms_per_step': ms, 'frames': frames,
           'c2_median_ms': {p: sorted(v)[len(v) // 2] for p, v in ms.items()}}
    med = out['c2_median_ms']
    out['speedup_bf16x3_vs_f32'] = round(med['f32'] / med['bf16x3'], 3)
    out['kernels_bf16x3'] = kernel_table(*runs['bf16x3'], 'bf16x3')
    out['kernels_f32'] = kernel_table(*runs['f32'], 'f32')
    del runs
    torch.cuda.empty_cache()
    if not args.no_inference:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from bench_inference import measure
        inf = measure('bf16x3')
        out['inference_c4_bf16x3'] = {'ms_per_batch': inf['graph_replay']['ms_per_batch'], 'eager': inf.get('eager')}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
