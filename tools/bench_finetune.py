"""One HiFi-GAN fine-tuning step (reference vocoder/finetune_hifigan.py:203-245) at the reference's training segment: B = 16 segments of
32 mel frames (8192 samples), synthetic weights, f32 operands.  One JSON line:

  * fused_ms: ``HiFiGanFineTuner.train_step`` -- weight norm, both AdamW steps and the re-fold in one ``dx_wn_adamw`` launch each;
  * composed_ms: the same step composed from the public API as it stood before the fine-tuner, with two ``torch.optim.AdamW``
    (INTEGRATION.md's earlier hand-assembled loop): ``generator(x)`` under autograd's weight norm, ``discriminator_backward``,
    ``optim_d.step``, ``refresh_weights``, ``generator_losses`` + ``MelL1Loss``, ``backward``, ``optim_g.step``;
  * the two ``dx_wn_adamw`` launches of one traced fused step: event time, the bytes ``profiling.price`` counts, GB/s.

Wall clock around synchronised calls and events around the launches, as DESIGN.md sections 17 / 18 took theirs.

    python tools/bench_finetune.py [v1|v2|v3] [--steps N]
    python tools/bench_finetune.py [v1|v2|v3] [--steps N] --data      # the cost of feeding the step: see data_mode
"""
import itertools
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tests import disc_helpers as dh  # noqa: E402
from tests import vocoder_helpers as vh  # noqa: E402
import ubisoft_laforge_daft_exprt_amd as pkg  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import _lib, profiling, vocoder as voc  # noqa: E402
from ubisoft_laforge_daft_exprt_amd.mel import MelL1Loss, MelSpectrogram  # noqa: E402

B, FRAMES = 16, 32


def timed(fn, n, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def synthetic_corpus(n_utt=256, seed=5):
    """``n_utt`` utterances of 3 to 5 s: random int16 audio and random mels, as ``HiFiGanFineTuneData.from_arrays`` takes them."""
    import numpy as np
    g = np.random.default_rng(seed)
    names, mels, wavs = [], [], []
    for u in range(n_utt):
        T = int(g.integers(258, 431))
        names.append(f'utt{u:04d}')
        mels.append((-5.0 + 2.0 * g.standard_normal((80, T))).astype(np.float32))
        wavs.append(g.integers(-20000, 20000, T * voc.HOP + int(g.integers(0, voc.HOP)), dtype=np.int16))
    return names, mels, wavs


def data_mode(name, steps, dev='cuda'):
    """``--data``: what feeding the step costs.  One JSON line:

      * batch_ms: events around ``data.batch`` (both launches), mean over ``--steps`` x 20 calls; ft_batch_launch / mel_launch: the two
        launches of one traced call, with the bytes ``profiling.price`` counts;
      * step_resident_ms / step_data_ms: ``train_step`` fed from tensors that stay on the device / from ``data.batch(step)``;
      * host_batch_ms: one process running the reference's per-item path as tests/finetune_data_helpers.py restates it (crop or pad,
        int16 -> float, the loss mel by torch.stft; from arrays in memory: no file is read) for B items, stacked, pinned and copied to
        the device, synchronised."""
    import numpy as np
    from tests import finetune_data_helpers as fh
    S = FRAMES * voc.HOP
    names, mels, wavs = synthetic_corpus()
    data = pkg.HiFiGanFineTuneData.from_arrays(names, mels, wavs, segment_size=S, batch_size=B, seed=1, device=dev)
    out = {'config': name, 'mode': 'data', 'workload': f'B={B} segments of {FRAMES} frames ({S} samples) from {len(names)} utterances, '
           f'{data.nbytes / 2 ** 20:.1f} MiB resident', 'steps': steps, 'steps_per_epoch': data.steps_per_epoch}
    calls = steps * 20
    for s in range(3):
        data.batch(s)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for s in range(calls):
        data.batch(s)
    b.record()
    torch.cuda.synchronize()
    out['batch_ms'] = round(a.elapsed_time(b) / calls, 4)
    recs = []
    old = _lib.set_timer(recs)
    data.batch(calls)
    torch.cuda.synchronize()
    _lib.set_timer(old)
    geom = profiling.Geometry([[FRAMES] * B])
    for tag, rec_name in (('ft_batch_launch', 'dx_ft_batch'), ('mel_launch', 'dx_mel')):
        _, args, e0, e1 = next(r for r in recs if r[0] == rec_name)
        ms, nbytes = e0.elapsed_time(e1), profiling.price(rec_name, args, geom)[3]
        out[tag] = {'ms': round(ms, 4), 'bytes': nbytes, 'gb_per_s': round(nbytes / ms / 1e6, 1) if nbytes else None}

    tuner = pkg.HiFiGanFineTuner({'generator': vh.state_dict(name)}, dh.state_dicts(), dev)
    x, y, y_mel = (t.clone() for t in data.batch(0)[:3])
    out['step_resident_ms'] = round(timed(lambda: tuner.train_step(x, y, y_mel), steps), 3)
    out['step_data_ms'] = round(timed(lambda: tuner.train_step(*data.batch(tuner.step)[:3]), steps), 3)
    out['step_resident_again_ms'] = round(timed(lambda: tuner.train_step(x, y, y_mel), steps), 3)

    order = data.epoch_order(0).tolist()
    g, position = np.random.default_rng(0), itertools.count()

    def host_batch():
        rows = order[(next(position) % data.steps_per_epoch) * B:][:B]
        items = []
        for u in rows:
            start = int(g.integers(0, data.max_start(u) + 1))
            hx, hy = fh.host_item(mels[u], wavs[u], start, S, voc.HOP)
            items.append((torch.from_numpy(hx), torch.from_numpy(hy), fh.host_loss_mel(hy)))
        return [torch.stack(col).pin_memory().to(dev, non_blocking=True) for col in zip(*items)]

    with torch.no_grad():
        out['host_batch_ms'] = round(timed(host_batch, steps * 4), 3)
    out['host_threads'] = torch.get_num_threads()
    print(json.dumps(out), flush=True)


def main():
    name = next((a for a in sys.argv[1:] if a in voc.CONFIGS), 'v1')
    steps = int(sys.argv[sys.argv.index('--steps') + 1]) if '--steps' in sys.argv else 5
    if '--data' in sys.argv:
        return data_mode(name, steps)
    dev = 'cuda'
    S = FRAMES * voc.HOP
    g = torch.Generator().manual_seed(3)
    x = ((torch.randn(B, 80, FRAMES, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0)).to(dev)
    y = dh.make_inputs(S, 9, B)[0].to(dev)
    y_mel, _, _ = MelSpectrogram(fmax=None, device=dev)(y[:, 0], [S] * B)
    gen_state, disc_state = {'generator': vh.state_dict(name)}, dh.state_dicts()
    out = {'config': name, 'workload': f'B={B} segments of {FRAMES} frames ({S} samples), f32', 'steps': steps}

    tuner = pkg.HiFiGanFineTuner(gen_state, disc_state, dev)
    out['fused_ms'] = round(timed(lambda: tuner.train_step(x, y, y_mel), steps), 3)
    recs = []
    torch.cuda.synchronize()
    old = _lib.set_timer(recs)
    tuner.train_step(x, y, y_mel)
    torch.cuda.synchronize()
    _lib.set_timer(old)
    geom = profiling.Geometry([[FRAMES] * B])
    for tag, (rec_name, args, a, b) in zip(('optim_d', 'optim_g'), [r for r in recs if r[0] == 'dx_wn_adamw']):
        ms = a.elapsed_time(b)
        nbytes = profiling.price(rec_name, args, geom)[3]
        out[f'{tag}_launch'] = {'ms': round(ms, 4), 'bytes': nbytes, 'gb_per_s': round(nbytes / ms / 1e6, 1)}
    by_name = {}
    for rec_name, _, a, b in recs:
        row = by_name.setdefault(rec_name, [0, 0.0])
        row[0] += 1
        row[1] += a.elapsed_time(b)
    out['fused_launches'] = {k: {'launches': n, 'ms': round(ms, 3)} for k, (n, ms) in sorted(by_name.items(), key=lambda kv: -kv[1][1])}
    del tuner
    torch.cuda.empty_cache()

    generator = pkg.HiFiGANGenerator(voc.CONFIGS[name]()).to(dev)
    generator.load_state_dict(gen_state['generator'])
    D, mel_l1 = pkg.HiFiGanDiscriminators(disc_state, dev), MelL1Loss(fmax=None, device=dev)
    optim_g = torch.optim.AdamW(generator.parameters(), 2e-4, betas=(0.8, 0.99))
    optim_d = torch.optim.AdamW(itertools.chain(D.msd.parameters(), D.mpd.parameters()), 2e-4, betas=(0.8, 0.99))

    def composed():
        y_g_hat = generator(x)
        optim_d.zero_grad()
        D.discriminator_backward(y, y_g_hat)
        optim_d.step()
        D.mpd.refresh_weights()
        D.msd.refresh_weights()
        optim_g.zero_grad()
        adv = D.generator_losses(y, y_g_hat)
        loss = adv['loss_gen_s'] + adv['loss_gen_f'] + adv['loss_fm_s'] + adv['loss_fm_f'] + mel_l1(y_g_hat[:, 0], [S] * B, y_mel)
        loss.backward()
        optim_g.step()

    out['composed_ms'] = round(timed(composed, steps), 3)
    out['composed_over_fused'] = round(out['composed_ms'] / out['fused_ms'], 3)
    out['peak_memory_mb'] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
