"""Training on a STREAM of batches whose padded shape changes every step (the reference's collate pads each batch to its own longest
utterance): K C2-sized batches ``synthetic_batch(**CONFIGS['C2'], seed=s)`` for distinct s, run through trainer.Trainer in three modes --

    exact     graphs keyed on each batch's exact (L_max, T_max) (Trainer(), the default): about one capture per step
    bucketed  graphs keyed on (L_max rounded up to 16, T_max rounded up to 64) (Trainer(bucket=(16, 64)))
    eager     no graphs (Trainer(use_graphs=False))

One JSON line per mode: captures, wall ms/step over the whole stream (captures included), steady-state replay ms/step (the mean of the
steps that replayed an existing graph) and torch.cuda.max_memory_allocated.  A last line prices the padding: bucketed replay against
exact-shape replay on the SAME batch (both graphs captured, then alternated).

    python tools/train_stream.py --steps 40 --precision bf16
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def _trainer(pkg, hp, dev, **kw):
    from ubisoft_laforge_daft_exprt_amd.loss import pitch_predictor_shapes
    from ubisoft_laforge_daft_exprt_amd.synth import synthetic_state_dict
    from ubisoft_laforge_daft_exprt_amd.trainer import Trainer
    model = pkg.DaftExprt(hp).to(dev)
    model.load_state_dict(synthetic_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1234))
    crit = pkg.DaftExprtLoss(dev, hp)
    crit.load_pitch_predictor(synthetic_state_dict(pitch_predictor_shapes(), 1235))
    return Trainer(model, crit, hp, **kw)


def _timed_step(trainer, batch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss, _, _ = trainer.train_step([batch])
    float(loss)                                    # the step's work is done when its loss can be read
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--precision', default='bf16', choices=['f32', 'bf16', 'bf16x3'])
    ap.add_argument('--modes', default='exact,bucketed,eager')
    ap.add_argument('--overhead-reps', type=int, default=10)
    args = ap.parse_args()
    import ubisoft_laforge_daft_exprt_amd as pkg
    from ubisoft_laforge_daft_exprt_amd.synth import CONFIGS, synthetic_batch
    dev = torch.device('cuda', 0)
    torch.cuda.init()
    torch.cuda.set_device(dev)
    pkg.set_precision(args.precision)
    hp = pkg.HyperParams(n_speakers=3)
    cfg = dict(CONFIGS['C2'], n_speakers=3)
    batches = [synthetic_batch(**{**cfg, 'seed': 5000 + s}) for s in range(args.steps)]
    shapes = {(b[0].shape[1], int(b[9].max())) for b in batches}
    kwargs = {'exact': dict(), 'bucketed': dict(bucket=(16, 64)), 'eager': dict(use_graphs=False)}
    for mode in args.modes.split(','):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        trainer = _trainer(pkg, hp, dev, **kwargs[mode])
        pkg.manual_seed(1234)
        captures, total, replay = 0, 0.0, []
        for b in batches:
            before = {id(g) for g in trainer.graphs.values()}
            ms = _timed_step(trainer, b)
            total += ms
            if any(id(g) not in before for g in trainer.graphs.values()):      # this step captured a new graph set
                captures += 1
            else:
                replay.append(ms)
        print(json.dumps({'mode': mode, 'precision': args.precision, 'steps': args.steps, 'distinct_exact_shapes': len(shapes),
                          'captures': captures, 'wall_ms_per_step': round(total / args.steps, 3),
                          'steady_ms_per_step': round(sum(replay) / max(1, len(replay)), 3) if replay else None,
                          'max_memory_allocated_mb': round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)}), flush=True)
        del trainer
    # the price of the padding on ONE batch: its exact-shape graph against its bucket's graph, replays alternated
    b = batches[0]
    te, tb = _trainer(pkg, hp, dev), _trainer(pkg, hp, dev, bucket=(16, 64))
    for t in (te, tb):
        for _ in range(3):
            _timed_step(t, b)                          # capture + warm replays
    ex, bu = [], []
    for _ in range(args.overhead_reps):
        ex.append(_timed_step(te, b))
        bu.append(_timed_step(tb, b))
    med = lambda v: sorted(v)[len(v) // 2]
    L, T = b[0].shape[1], int(b[9].max())
    print(json.dumps({'padding_overhead': True, 'exact_shape': [L, T], 'bucket_shape': [-(-L // 16) * 16, -(-T // 64) * 64],
                      'exact_replay_ms': round(med(ex), 3), 'bucketed_replay_ms': round(med(bu), 3),
                      'overhead_pct': round(100.0 * (med(bu) / med(ex) - 1.0), 2)}), flush=True)


if __name__ == '__main__':
    main()
