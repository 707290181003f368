"""Writes tests/golden/discriminators_train_<T>.npz from the REFERENCE HiFi-GAN discriminators, with autograd to every parameter.

Runs only in the build container, where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.
Same weights and inputs as make_golden_discriminators.py (``disc_helpers.state_dicts()`` / ``inputs(T)``), the weight and spectral
norms KEPT and the modules in ``.eval()``: no power iteration runs, but autograd still flows through sigma = u . (W v) with the stored
u and v -- ``discriminator_loss_grad(..., power_iterations=0)``.  Per length T in (12, 257, 2048), batch 2, in float64 and in float32:

    (loss_disc_s + loss_disc_f).backward()                                  (finetune_hifigan.py:216-226)

and one file per length holds ``losses64`` (loss_disc_f, loss_disc_s, float64), per parameter ``<mpd|msd>/<key>/norm`` (the gradient's
L2 norm: float64 run, float32 run), ``.../g64`` and ``.../g32`` (the gradient at ``disc_helpers.sample_index(numel)``), and ``eps``: the
step of the plain descent test, 2e-3 loss / |g|^2, so that the float64 gradient predicts a decrease of 2e-3 of the loss, far above fp32
noise.  Fixed zip timestamps: a rerun reproduces the files bit for bit.

    python tests/golden/make_golden_discriminators_train.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from tests import disc_helpers as dh  # noqa: E402
import make_golden_discriminators as fwd  # noqa: E402

torch.set_num_threads(8)


def main():
    ref = fwd._load_reference()
    states = dh.state_dicts()

    def load(dtype):                       # a weight-normed module cannot be deep-copied: each precision gets modules of its own
        mods = {'mpd': ref.MultiPeriodDiscriminator(), 'msd': ref.MultiScaleDiscriminator()}
        for d, m in mods.items():
            m.load_state_dict(states[d], strict=True)
            m.to(dtype).eval()
        return mods

    models, models64 = load(torch.float32), load(torch.float64)
    for T in dh.LENGTHS:
        y, y_hat = dh.inputs(T)
        rec, grads = {}, {}
        for tag, mods, dtype in (('64', models64, torch.float64), ('32', models, torch.float32)):
            for m in mods.values():
                m.zero_grad(set_to_none=True)
            yy, x = y.to(dtype), y_hat.to(dtype).detach()
            dr_f, dg_f, _, _ = mods['mpd'](yy, x)
            loss_f = ref.discriminator_loss(dr_f, dg_f)[0]
            dr_s, dg_s, _, _ = mods['msd'](yy, x)
            loss_s = ref.discriminator_loss(dr_s, dg_s)[0]
            (loss_s + loss_f).backward()
            grads[tag] = {f'{d}/{k}': q.grad.detach().clone() for d, m in mods.items() for k, q in m.named_parameters()}
            if tag == '64':
                rec['losses64'] = np.array([float(loss_f.detach()), float(loss_s.detach())], dtype=np.float64)
        assert len(grads['64']) == 154 and list(grads['64']) == list(grads['32'])
        sq = 0.0
        for key, g64 in grads['64'].items():
            g32 = grads['32'][key]
            idx = torch.from_numpy(dh.sample_index(g64.numel()))
            rec[key + '/norm'] = np.array([float(g64.norm()), float(g32.double().norm())], dtype=np.float64)
            rec[key + '/g64'] = g64.flatten()[idx].numpy().copy()
            rec[key + '/g32'] = g32.flatten()[idx].numpy().copy()
            sq += float(g64.norm()) ** 2
        rec['eps'] = np.array(2e-3 * rec['losses64'].sum() / sq, dtype=np.float64)
        for d in ('mpd', 'msd'):
            a = torch.cat([torch.from_numpy(rec[k + '/g64']) for k in grads['64'] if k.startswith(d)])
            b = torch.cat([torch.from_numpy(rec[k + '/g32']).double() for k in grads['64'] if k.startswith(d)])
            print(f'T {T} {d}: sampled f32 vs f64 relative L2 {float((a - b).norm() / a.norm()):.3e}')
        path = os.path.join(HERE, f'discriminators_train_{T}.npz')
        fwd._write_npz(path, rec)
        print(f"T {T}: losses {rec['losses64']}, |g|^2 {sq:.4e}, eps {float(rec['eps']):.4e}; wrote {os.path.getsize(path)} bytes")


if __name__ == '__main__':
    main()
