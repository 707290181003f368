"""Writes tests/golden/discriminators_manifest.json and tests/golden/discriminators.npz from the REFERENCE HiFi-GAN discriminators.

Runs only in the build container, where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.
The weights are not stored: they are ``synthetic_state_dict(manifest shapes, 1234)`` loaded with ``load_state_dict(strict=True)``.
One exception: a synthetic ``weight_u`` / ``weight_v`` makes the spectral norm's sigma tiny (the outputs of the spectral-normed
sub-discriminator reach 1e13), so that sub-discriminator is run 30 times in train mode -- one power iteration each -- and the
resulting ``u`` and ``v`` of its 8 layers are stored in the fixture (``sn/<key>``); tests/disc_helpers.py overlays them.

Both norms are then removed (``remove_weight_norm`` / ``remove_spectral_norm``: the eval-mode weights, in fp32) and the SAME folded
fp32 weights run in fp32 (the golden values) and in fp64: the spread between the two is what the parity bars are set against.

Per length T in (12, 257, 2048), batch 2: the inputs, every score in full, per feature map 256 values at fixed flat indices
(tests/disc_helpers.sample_index) plus [mean r, mean |r|, mean g, mean |g|, spread max, spread mean, max |f64|], and every loss term
in fp32 and fp64.  The archive is written with fixed zip timestamps, so a rerun reproduces the file bit for bit.

    python tests/golden/make_golden_discriminators.py
"""
import copy
import importlib.util
import io
import json
import os
import sys
import zipfile

sys.dont_write_bytecode = True

import numpy as np
import torch
from torch.nn.utils import remove_spectral_norm, remove_weight_norm

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = '/root/reference/src/daft_exprt/vocoder/discriminators.py'

from tests import disc_helpers as dh  # noqa: E402

SEED = 1234
POWER_ITERATIONS = 30
torch.set_num_threads(8)


def _load_reference():
    spec = importlib.util.spec_from_file_location('ref_discriminators', REF)     # the module imports only torch
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_npz(path, rec):
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(rec[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def _remove_norms(model):
    for m in model.modules():
        if isinstance(m, (torch.nn.Conv1d, torch.nn.Conv2d)):
            if hasattr(m, 'weight_orig'):
                remove_spectral_norm(m)
            else:
                remove_weight_norm(m)


def _stats(r32, g32, r64, g64):
    d = torch.cat([(r32.double() - r64).abs().flatten(), (g32.double() - g64).abs().flatten()])
    return np.array([r32.double().mean(), r32.double().abs().mean(), g32.double().mean(), g32.double().abs().mean(),
                     d.max(), d.mean(), max(r64.abs().max(), g64.abs().max())], dtype=np.float64)


def main():
    ref = _load_reference()
    models = {'mpd': ref.MultiPeriodDiscriminator(), 'msd': ref.MultiScaleDiscriminator()}
    man = {'seed': SEED, 'power_iterations': POWER_ITERATIONS}
    for d, m in models.items():
        man[d] = {k: list(v.shape) for k, v in m.state_dict().items()}
    with open(os.path.join(HERE, 'discriminators_manifest.json'), 'w') as f:
        json.dump(man, f, indent=1)
    states = dh.synthetic_states(man)
    for d, m in models.items():
        m.load_state_dict(states[d], strict=True)
    rec = {}
    # the spectral-normed sub-discriminator: power iterations in train mode, on the longest fixture input
    sn = models['msd'].discriminators[0].train()
    y_it, _ = dh.make_inputs(max(dh.LENGTHS), SEED)
    with torch.no_grad():
        for _ in range(POWER_ITERATIONS):
            sn(y_it)
    for k, v in models['msd'].state_dict().items():
        if k.startswith('discriminators.0.') and k.endswith(('weight_u', 'weight_v')):
            rec['sn/' + k] = v.detach().numpy().copy()
    for m in models.values():
        m.eval()
        _remove_norms(m)
    models64 = {d: copy.deepcopy(m).double().eval() for d, m in models.items()}
    for T in dh.LENGTHS:
        y, y_hat = dh.make_inputs(T, SEED)
        rec[f'{T}/y'], rec[f'{T}/y_hat'] = y.numpy(), y_hat.numpy()
        for d in ('mpd', 'msd'):
            with torch.no_grad():
                o32 = models[d](y, y_hat)
                o64 = models64[d](y.double(), y_hat.double())
            for i in range(len(o32[0])):
                rec[f'{T}/{d}/{i}/score_r'], rec[f'{T}/{d}/{i}/score_g'] = o32[0][i].numpy(), o32[1][i].numpy()
                for j in range(len(o32[2][i])):
                    r32, g32, r64, g64 = o32[2][i][j], o32[3][i][j], o64[2][i][j], o64[3][i][j]
                    idx = torch.from_numpy(dh.sample_index(r32.numel()))
                    rec[f'{T}/{d}/{i}/fmap{j}/shape'] = np.array(r32.shape, dtype=np.int64)
                    rec[f'{T}/{d}/{i}/fmap{j}/r'] = r32.flatten()[idx].numpy()
                    rec[f'{T}/{d}/{i}/fmap{j}/g'] = g32.flatten()[idx].numpy()
                    rec[f'{T}/{d}/{i}/fmap{j}/stats'] = _stats(r32, g32, r64, g64)
            # every loss term, fp32 (as the reference computes it) and fp64: [total, per-sub-discriminator terms ...]
            for tag, o in (('f32', o32), ('f64', o64)):
                dl, rl, gl = ref.discriminator_loss(o[0], o[1])
                gen, gens = ref.generator_loss(o[1])
                fm = ref.feature_loss(o[2], o[3])
                fms = [torch.mean(torch.abs(a - b)) for dr, dg in zip(o[2], o[3]) for a, b in zip(dr, dg)]
                rec[f'{T}/{d}/loss/{tag}/disc'] = np.array([float(dl)] + [float(v) for v in rl] + [float(v) for v in gl], dtype=np.float64)
                rec[f'{T}/{d}/loss/{tag}/gen'] = np.array([float(gen)] + [float(v) for v in gens], dtype=np.float64)
                rec[f'{T}/{d}/loss/{tag}/fm'] = np.array([float(fm)] + [float(v) for v in fms], dtype=np.float64)
            worst = max(rec[f'{T}/{d}/{i}/fmap{j}/stats'][4] / rec[f'{T}/{d}/{i}/fmap{j}/stats'][6]
                        for i in range(len(o32[0])) for j in range(len(o32[2][i])))
            print(f'T {T} {d}: score max {max(float(s.abs().max()) for s in o32[0]):.3f}, worst f32-vs-f64 spread / max|f64| {worst:.2e}, '
                  f"losses {rec[f'{T}/{d}/loss/f32/disc'][0]:.5f} {rec[f'{T}/{d}/loss/f32/gen'][0]:.5f} {rec[f'{T}/{d}/loss/f32/fm'][0]:.5f}")
    _write_npz(os.path.join(HERE, 'discriminators.npz'), rec)
    print('wrote', os.path.getsize(os.path.join(HERE, 'discriminators.npz')), 'bytes')


if __name__ == '__main__':
    main()
