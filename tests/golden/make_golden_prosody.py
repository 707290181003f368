"""Writes tests/golden/prosody.npz from the REFERENCE prosody code on CPU.

Runs only where /root/reference is mounted; nothing under tests/ reads /root/reference at test time.  The reference modules are loaded
from their files under an empty parent package (so daft_exprt/__init__.py never runs), absent third-party modules stubbed.  Called:

  extract_features.get_symbols_energy / get_symbols_pitch     the symbol means (text with three decimals, parsed back)
  generate.generate_batch_mel_specs                           lines 213-278 as they stand -- host durations with alpha_dur, the
      speaker-statistics lookup with its 'spk 0' fallback, _normalize_external_feature, alpha scaling -- by handing it a collate stub
      and a model stub whose ``inference`` keeps the ``external_tensors`` it is given and stops the call
  model.DaftExprt.pitch_shift / pitch_multiply                after model.py:1077-1080 (factors, zero where durations_int == 0), which
      are restated here in the same torch operations

Per case: inputs, the reference's fp32 result, the float64 restatement (tests/prosody_helpers.py) and spread = |fp32 - f64| as
[energy max, energy mean, pitch max, pitch mean].  For the committed inference goldens (inference_add / inference_multiply) the
float64 restatement of their stored energy / pitch predictions and the spread of the stored values are added, so that an end-to-end
test has a bar for them.  Arrays only.

    python tests/golden/make_golden_prosody.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
SRC = '/root/reference/src/daft_exprt'

from tests import prosody_helpers as ph  # noqa: E402

torch.set_num_threads(8)

SPEAKER_STATS = np.array([[2.0, 1.5, 5.0, 0.25], [1.7, 1.1, 4.6, 0.3]])        # 'spk 0', 'spk 1': energy mean / std, pitch mean / std
SOURCE_STATS = np.array([2.4, 1.3, 4.8, 0.28])
SPEAKER_IDS = [0, 1, 5, 1]                                                      # 5 has no statistics: 'spk 0' stands in
E2E_PITCH_STATS = np.array([[5.0, 0.25], [4.6, 0.3]])                           # the stats the inference goldens were captured with


class _Anything(types.ModuleType):
    """A stand-in for an absent third-party module: every attribute is another stand-in."""
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        mod = _Anything(f'{self.__name__}.{name}')
        setattr(self, name, mod)
        return mod

    def __call__(self, *args, **kwargs):
        return self


def _load_reference():
    pkg = types.ModuleType('daft_exprt')
    pkg.__path__ = [SRC]
    sys.modules['daft_exprt'] = pkg
    while True:                                              # stub whatever third-party module is absent here; none is called on this path
        try:
            from daft_exprt import extract_features, generate
            from daft_exprt.model import DaftExprt
            break
        except ModuleNotFoundError as exc:
            if not exc.name or exc.name.startswith('daft_exprt') or exc.name in sys.modules:
                raise
            sys.modules[exc.name] = _Anything(exc.name)
            for half in [k for k in sys.modules if k.startswith('daft_exprt.')]:      # drop half-imported reference modules
                del sys.modules[half]
    return extract_features, generate, DaftExprt


def _stats(table, ids=()):
    st = {f'spk {i}': {'energy': {'mean': float(r[0]), 'std': float(r[1])}, 'pitch': {'mean': float(r[2]), 'std': float(r[3])}}
          for i, r in enumerate(table)}
    for i in ids:
        st.setdefault(f'spk {i}', st['spk 0'])
    return st


class _Captured(Exception):
    pass


def reference_external_tensors(gen, entries, lens, source_stats, alpha_dur, alpha_pitch, alpha_energy):
    """generate.py:213-278 run as it stands; returns the external_tensors dict it hands to model.inference."""
    B, L = len(entries), max(lens)
    hp = types.SimpleNamespace(hop_length=256, sampling_rate=22050, stats=_stats(SPEAKER_STATS))
    collated = (torch.zeros(B, L, dtype=torch.long), torch.ones(B, L), torch.ones(B, L), torch.zeros(B, L), torch.tensor(lens),
                torch.tensor(SPEAKER_IDS), [f'utt{b}' for b in range(B)], entries)

    class Model:
        def parameters(self):
            return iter([torch.zeros(1)])

        def inference(self, inputs, pitch_transform, hparams, external_tensors, **kw):
            raise _Captured(external_tensors)

    keep_collate, keep_cuda = gen.collate_tensors, torch.Tensor.cuda
    gen.collate_tensors = lambda *a, **k: collated
    torch.Tensor.cuda = lambda self, *a, **k: self           # the reference moves its tensors to the model's device: the CPU here
    try:
        gen.generate_batch_mel_specs(Model(), [''] * B, None, None, None, 'add', list(SPEAKER_IDS), [f'utt{b}' for b in range(B)], None, hp, 1,
                                     batch_external_prosody=entries, source_stats=source_stats, alpha_dur=alpha_dur, alpha_pitch=alpha_pitch,
                                     alpha_energy=alpha_energy)
    except _Captured as c:
        return c.args[0]
    finally:
        gen.collate_tensors, torch.Tensor.cuda = keep_collate, keep_cuda
    raise AssertionError('the reference did not reach model.inference')


def symbol_case(ef, rec):
    g = np.random.default_rng(4321)
    B, L = 3, 37
    in_lens = [37, 20, 1]
    dur = np.zeros((B, L), dtype=np.int64)
    dur[0, :37] = g.integers(1, 9, 37)
    dur[0, [0, 36, 10, 11]] = 0                               # first, last, two in a row
    dur[0, 3], dur[0, 7], dur[0, 20], dur[0, 15] = 1, 70, 300, 6
    dur[1, :20] = g.integers(1, 9, 20)
    dur[1, [0, 19, 5, 6]] = 0
    dur[1, 2] = 70
    dur[2, 0] = 5
    T = int(dur[0].sum())                                     # row 0 uses every frame, rows 1 and 2 stop short
    assert dur[1].sum() < T
    fe = (np.abs(g.standard_normal((B, T))) * 3 + 0.1).astype(np.float32)
    fp = (5.0 + 0.3 * g.standard_normal((B, T))).astype(np.float32)
    fp[g.random((B, T)) < 0.25] = 0.0
    off15 = int(dur[0, :15].sum())
    fp[0, off15:off15 + 6] = 0.0                              # symbol 15 of row 0: every frame unvoiced
    ref_e, ref_p, e32, p32 = (np.zeros((B, L)) for _ in range(4))
    for b in range(B):
        n, tot = in_lens[b], int(dur[b].sum())
        markers = [[0.0, 0.0, int(d), 'a', 'w', 0] for d in dur[b, :n]]
        ref_e[b, :n] = [float(s) for s in ef.get_symbols_energy(fe[b, :tot], markers)]
        ref_p[b, :n] = [float(s) for s in ef.get_symbols_pitch(fp[b, :tot], markers)]
        idx = 0
        for l in range(n):                                    # the same means before the reference turns them into text
            d = int(dur[b, l])
            if d:
                e32[b, l] = np.mean(fe[b, idx:idx + d])
                v = fp[b, idx:idx + d]
                v = v[v > 0.]
                p32[b, l] = np.mean(v) if len(v) else 0.0
                idx += d
    e64, p64 = ph.symbol_means64(fe, fp, dur, in_lens)
    assert np.abs(ref_e - e64).max() <= 5.01e-4 and np.abs(ref_p - p64).max() <= 5.01e-4
    de, dp = np.abs(e32 - e64), np.abs(p32 - p64)
    rec.update({'sym/frames_energy': fe, 'sym/frames_pitch': fp, 'sym/dur_int': dur, 'sym/in_lens': np.array(in_lens),
                'sym/energy_ref3': ref_e, 'sym/pitch_ref3': ref_p, 'sym/energy_ref32': e32.astype(np.float32), 'sym/pitch_ref32': p32.astype(np.float32),
                'sym/energy_f64': e64, 'sym/pitch_f64': p64, 'sym/spread': np.array([de.max(), de.mean(), dp.max(), dp.mean()])})
    print(f'symbol means: T {T}  |np.mean fp32 - f64| energy max {de.max():.2e} pitch max {dp.max():.2e}')


def conditioning_cases(gen, DaftExprt, rec):
    g = np.random.default_rng(2468)
    B, L = 4, 70
    in_lens = [70, 64, 33, 1]
    energy = (np.abs(g.standard_normal((B, L))) * 1.5 + 0.2).astype(np.float32)
    pitch = (4.8 + 0.28 * g.standard_normal((B, L))).astype(np.float32)
    energy[g.random((B, L)) < 0.25] = 0.0
    pitch[g.random((B, L)) < 0.25] = 0.0
    pitch[2] = 0.0                                            # an all-unvoiced row
    frames = (g.random((B, L)) * 11 + 0.6).astype(np.float32)
    frames[g.random((B, L)) < 0.12] = 0.0
    e_fac = (0.6 + 0.8 * g.random((B, L))).astype(np.float32)
    p_fac = {'add': (-20 + 60 * g.random((B, L))).astype(np.float32), 'multiply': (-0.5 + 2 * g.random((B, L))).astype(np.float32)}
    for a in (energy, pitch, frames, e_fac, p_fac['add'], p_fac['multiply']):
        for b, n in enumerate(in_lens):
            a[b, n:] = 0.0
    entries = [{'symbols': ['a'] * n, 'durations_frames': frames[b, :n].tolist(), 'energy': energy[b, :n].tolist(), 'pitch': pitch[b, :n].tolist()}
               for b, n in enumerate(in_lens)]
    source = {'energy': {'mean': SOURCE_STATS[0], 'std': SOURCE_STATS[1]}, 'pitch': {'mean': SOURCE_STATS[2], 'std': SOURCE_STATS[3]}}
    rec.update({'cond/energy': energy, 'cond/pitch': pitch, 'cond/durations_frames': frames, 'cond/in_lens': np.array(in_lens),
                'cond/speaker_ids': np.array(SPEAKER_IDS), 'cond/speaker_stats': SPEAKER_STATS, 'cond/source_stats': SOURCE_STATS,
                'cond/energy_factors': e_fac, 'cond/pitch_factors_add': p_fac['add'], 'cond/pitch_factors_multiply': p_fac['multiply']})
    # host durations: generate.py:226-236 for three alpha_dur
    for alpha_dur in (1.0, 1.3, 0.5):
        ext = reference_external_tensors(gen, entries, in_lens, None, alpha_dur, 1.0, 1.0)
        rec[f'dur/a{alpha_dur}/seconds'] = ext['duration_preds'].numpy()
        rec[f'dur/a{alpha_dur}/int'] = ext['durations_int'].numpy()
    dur_int = rec['dur/a1.0/int']
    rec['cond/dur_int'] = dur_int
    assert (dur_int[0, :70] == 0).any()
    hp = types.SimpleNamespace(stats=_stats(SPEAKER_STATS, SPEAKER_IDS))        # pitch_shift has no fallback of its own
    stats_rows = np.stack([SPEAKER_STATS[i] if i < 2 else SPEAKER_STATS[0] for i in SPEAKER_IDS])

    def model_stage(e_norm, p_norm, mode):
        """model.py:1077-1087 on normalised prosody: the reference's fp32 energy / pitch predictions."""
        e = torch.from_numpy(e_norm).clone() * torch.from_numpy(e_fac)
        p = torch.from_numpy(p_norm).clone()
        d = torch.from_numpy(dur_int)
        e[d == 0] = 0.
        p[d == 0] = 0.
        if mode == 'add':
            p = DaftExprt.pitch_shift(None, p, torch.from_numpy(p_fac['add']), hp, torch.tensor(SPEAKER_IDS))
        else:
            p = DaftExprt.pitch_multiply(None, p, torch.from_numpy(p_fac['multiply']))
        return e.numpy(), p.numpy()

    names = []

    def store(name, e_ref, p_ref, e64, p64):
        assert not np.isnan(e_ref).any() and not np.isnan(p_ref).any(), name
        de, dp = np.abs(e_ref - e64), np.abs(p_ref - p64)
        spread = np.array([de.max(), de.mean(), dp.max(), dp.mean()])
        rec.update({f'cond/{name}/energy_ref': e_ref, f'cond/{name}/pitch_ref': p_ref, f'cond/{name}/energy_f64': e64, f'cond/{name}/pitch_f64': p64,
                    f'cond/{name}/spread': spread})
        names.append(name)
        print(f'{name:24s} |ref32 - f64| energy max {de.max():.2e} mean {de.mean():.2e}  pitch max {dp.max():.2e} mean {dp.mean():.2e}')

    for src in (0, 1):
        for alpha in (1.0, 1.3):
            ext = reference_external_tensors(gen, entries, in_lens, source if src else None, 1.0, alpha, alpha)
            e_norm, p_norm = ext['energy_preds'].numpy(), ext['pitch_preds'].numpy()
            if not src and alpha == 1.0:
                rec['cond/norm_energy'], rec['cond/norm_pitch'] = e_norm, p_norm
            for mode in ('add', 'multiply'):
                e_ref, p_ref = model_stage(e_norm, p_norm, mode)
                e64, p64 = ph.condition64(energy, pitch, dur_int, in_lens, e_fac, p_fac[mode], stats_rows, SOURCE_STATS if src else None,
                                          alpha, alpha, mode, True)
                store(f'src{src}_a{alpha}_{mode}', e_ref, p_ref, e64, p64)
    for mode in ('add', 'multiply'):                           # plain model.inference pre-processing of already normalised prosody
        e_ref, p_ref = model_stage(rec['cond/norm_energy'], rec['cond/norm_pitch'], mode)
        e64, p64 = ph.condition64(rec['cond/norm_energy'], rec['cond/norm_pitch'], dur_int, in_lens, e_fac, p_fac[mode], stats_rows, None,
                                  1.0, 1.0, mode, False)
        store(f'inference_{mode}', e_ref, p_ref, e64, p64)
    rec['cond/cases'] = np.array(names)


def end_to_end_bars(rec):
    """The committed inference goldens: float64 restatement of their stored energy / pitch predictions and the stored values' spread."""
    rec['e2e/pitch_stats'] = E2E_PITCH_STATS
    for mode in ('add', 'multiply'):
        z = np.load(os.path.join(HERE, f'inference_{mode}.npz'))
        ids = z['in/speaker_ids'].tolist()
        stats = np.array([[0.0, 1.0, *E2E_PITCH_STATS[i]] for i in ids])
        e64, p64 = ph.condition64(z['in/prosody_energy_preds'], z['in/prosody_pitch_preds'], z['out/durations_int'], z['in/input_lengths'],
                                  z['in/energy_factors'], z['in/pitch_factors'], stats, None, 1.0, 1.0, mode, False)
        de, dp = np.abs(z['out/energy_preds'] - e64), np.abs(z['out/pitch_preds'] - p64)
        rec[f'e2e/inference_{mode}/energy_f64'], rec[f'e2e/inference_{mode}/pitch_f64'] = e64, p64
        rec[f'e2e/inference_{mode}/spread'] = np.array([de.max(), de.mean(), dp.max(), dp.mean()])
        print(f'inference_{mode} golden: stored vs f64 energy max {de.max():.2e}  pitch max {dp.max():.2e}')


def main():
    ef, gen, DaftExprt = _load_reference()
    rec = {}
    symbol_case(ef, rec)
    conditioning_cases(gen, DaftExprt, rec)
    end_to_end_bars(rec)
    np.savez_compressed(os.path.join(HERE, 'prosody.npz'), **rec)
    print('prosody.npz:', os.path.getsize(os.path.join(HERE, 'prosody.npz')), 'bytes')


if __name__ == '__main__':
    main()
