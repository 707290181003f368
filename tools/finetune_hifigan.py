"""Fine-tune a HiFi-GAN vocoder on (predicted mel, ground-truth audio) pairs: the reference's vocoder/finetune_hifigan.py command line
on ``HiFiGanFineTuneData`` (the corpus resident on the device) and ``HiFiGanFineTuner.fit``.

    python tools/finetune_hifigan.py --fine_tuning_dir DIR --gen_checkpoint g_02500000_v1_uni --disc_checkpoint do_02500000 \\
        --output_dir cp_hifigan_ft --training_steps 5000

Differences from the reference's tool: ``--disc_checkpoint`` is required (this package has no initialiser for the discriminators);
``--num_workers`` is accepted and ignored (no host worker touches a batch); there is no TensorBoard and ``--summary_interval`` is
ignored: the step log goes to stdout every ``--stdout_interval`` steps; ``--seed`` and ``--segment_size`` are additions.  A tuner restored
with its optimisers continues from the checkpoint's step count: ``--training_steps`` is the count to reach, not the number to add.
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import ubisoft_laforge_daft_exprt_amd as pkg  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser(description='Fine-tune HiFi-GAN vocoder on Daft-Exprt TTS outputs (gfx950)')
    p.add_argument('--fine_tuning_dir', required=True, help='Directory with mel (.npy) / audio (.wav) pairs')
    p.add_argument('--gen_checkpoint', required=True, help='Pretrained generator checkpoint (weight norm intact)')
    p.add_argument('--disc_checkpoint', required=True, help='Pretrained discriminator checkpoint (do_*)')
    p.add_argument('--output_dir', default='cp_hifigan_ft', help='Directory for checkpoints')
    p.add_argument('--training_steps', type=int, default=5000)
    p.add_argument('--batch_size', type=int, default=16)
    p.add_argument('--learning_rate', type=float, default=0.0002)
    p.add_argument('--adam_b1', type=float, default=0.8)
    p.add_argument('--adam_b2', type=float, default=0.99)
    p.add_argument('--lr_decay', type=float, default=0.999)
    p.add_argument('--val_split', type=float, default=0.1)
    p.add_argument('--num_workers', type=int, default=4, help='accepted and ignored: batches are assembled on the device')
    p.add_argument('--reset_optimizers', action='store_true', help='Ignore the optimiser state, step and epoch of the disc checkpoint')
    p.add_argument('--save_disc', action='store_true', help='Also save the discriminators and optimisers (needed to resume)')
    p.add_argument('--stdout_interval', type=int, default=5)
    p.add_argument('--summary_interval', type=int, default=10, help='accepted and ignored: there is no TensorBoard')
    p.add_argument('--validation_interval', type=int, default=1000)
    p.add_argument('--checkpoint_interval', type=int, default=1000)
    p.add_argument('--segment_size', type=int, default=8192)
    p.add_argument('--seed', type=int, default=1234, help='seed of the pass orders and the crop draws')
    args = p.parse_args(argv)

    data = pkg.HiFiGanFineTuneData(args.fine_tuning_dir, segment_size=args.segment_size, val_split=args.val_split,
                                   batch_size=args.batch_size, seed=args.seed)
    print(f'Dataset: {len(data.train_names)} train, {len(data.val_names)} val (total {len(data.names)} pairs), '
          f'{data.nbytes / 2 ** 20:.1f} MiB on the device, {data.steps_per_epoch} steps per pass', flush=True)
    tuner = pkg.HiFiGanFineTuner(args.gen_checkpoint, args.disc_checkpoint, learning_rate=args.learning_rate,
                                 adam_b1=args.adam_b1, adam_b2=args.adam_b2, lr_decay=args.lr_decay, reset_optimizers=args.reset_optimizers)
    t0 = time.time()
    last = [t0, tuner.step]

    def log(step, losses):
        if args.stdout_interval and step % args.stdout_interval == 0:
            v = dict(losses.items())                                  # the one host transfer of this step
            now = time.time()
            gen = v['loss_gen_s'] + v['loss_gen_f'] + v['loss_fm_s'] + v['loss_fm_f'] + v['loss_mel']
            print(f"Step {step} | Gen {gen:.3f} | Disc {v['loss_disc_f'] + v['loss_disc_s']:.3f} | Mel L1 {v['loss_mel'] / 45:.4f} | "
                  f'{(now - last[0]) / max(1, step - last[1]):.3f} s/batch | {now - t0:.1f} s elapsed', flush=True)
            last[:] = [now, step]

    result = tuner.fit(data, args.training_steps, output_dir=args.output_dir, validation_interval=args.validation_interval,
                       checkpoint_interval=args.checkpoint_interval, save_disc=args.save_disc, log=log)
    for step, err in result.validation.items():
        print(f'Validation @ step {step} | Mel L1 {err:.4f}')
    print(f'Fine-tuning finished after {result.steps} steps at step {tuner.step} (epoch {tuner.epoch}); checkpoints in {args.output_dir}')


if __name__ == '__main__':
    main()
