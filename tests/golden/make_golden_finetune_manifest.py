"""Writes tests/golden/finetune_checkpoint_manifest.json: names, shapes and settings of the reference's fine-tuning checkpoints.

Runs only in the build container, where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.
The reference's ``HiFiGANGenerator`` (V1), ``MultiPeriodDiscriminator`` and ``MultiScaleDiscriminator`` on the CPU, the two ``AdamW`` and
``ExponentialLR`` as vocoder/finetune_hifigan.py:130-152 builds them (the script's defaults: learning_rate 2e-4, adam_b1 0.8, adam_b2
0.99, lr_decay 0.999, last_epoch -1), one step on zero gradients so that the optimiser state exists, then the two dicts of
``save_checkpoint`` (:88-107).  The manifest holds no weights: the key lists of ``g_*`` and ``do_*``, every ``param_groups[0]`` entry
with its value (``params`` as a count), the keys of one state entry, and per optimiser the state shapes in order.

    python tests/golden/make_golden_finetune_manifest.py
"""
import importlib.util
import itertools
import json
import os
import sys

sys.dont_write_bytecode = True

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VOCODER = os.path.join(os.environ.get('DAFT_EXPRT_REFERENCE', '/root/reference'), 'src', 'daft_exprt', 'vocoder')
ARGS = dict(learning_rate=2e-4, adam_b1=0.8, adam_b2=0.99, lr_decay=0.999)


def _load(name):
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(VOCODER, name + '.py'))     # both import only torch / numpy / stdlib
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _optimizer_entry(optim):
    sd = optim.state_dict()
    group = dict(sd['param_groups'][0])
    group['params'] = len(group['params'])
    group['betas'] = list(group['betas'])
    first = sd['state'][0]
    return {'n_param_groups': len(sd['param_groups']), 'param_group': group, 'state_keys': list(first),
            'step': float(first['step']), 'step_is_tensor': torch.is_tensor(first['step']),
            'shapes': [list(sd['state'][i]['exp_avg'].shape) for i in range(len(sd['state']))]}


def main():
    hifigan, disc = _load('hifigan'), _load('discriminators')
    generator = hifigan.HiFiGANGenerator(hifigan.DEFAULT_CONFIG)
    mpd, msd = disc.MultiPeriodDiscriminator(), disc.MultiScaleDiscriminator()
    optim_g = torch.optim.AdamW(generator.parameters(), lr=ARGS['learning_rate'], betas=(ARGS['adam_b1'], ARGS['adam_b2']))
    optim_d = torch.optim.AdamW(itertools.chain(msd.parameters(), mpd.parameters()), lr=ARGS['learning_rate'],
                                betas=(ARGS['adam_b1'], ARGS['adam_b2']))
    schedulers = [torch.optim.lr_scheduler.ExponentialLR(o, gamma=ARGS['lr_decay'], last_epoch=-1) for o in (optim_g, optim_d)]
    for o in (optim_g, optim_d):
        for group in o.param_groups:
            for p in group['params']:
                p.grad = torch.zeros_like(p)
        o.step()
    g_file = {'generator': generator.state_dict()}
    do_file = {'mpd': mpd.state_dict(), 'msd': msd.state_dict(), 'optim_g': optim_g.state_dict(), 'optim_d': optim_d.state_dict(),
               'steps': 1, 'epoch': 1}
    shapes = lambda sd: {k: list(v.shape) for k, v in sd.items()}
    manifest = {'args': ARGS, 'torch': torch.__version__.split('+')[0], 'n_schedulers': len(schedulers),
                'g': {'keys': list(g_file), 'generator': shapes(g_file['generator'])},
                'do': {'keys': list(do_file), 'mpd': shapes(do_file['mpd']), 'msd': shapes(do_file['msd'])},
                'optim_g': _optimizer_entry(optim_g), 'optim_d': _optimizer_entry(optim_d)}
    with open(os.path.join(HERE, 'finetune_checkpoint_manifest.json'), 'w') as f:
        json.dump(manifest, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
