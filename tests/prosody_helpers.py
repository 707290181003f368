"""Fixture loading and float64 numpy restatements for the prosody tests (data only; nothing here touches the reference tree).
tests/test_prosody_cpu.py pins these restatements to tests/golden/prosody.npz; the GPU tests then use them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'prosody.npz')
MODES = {'none': 0, 'add': 1, 'multiply': 2}


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def stats_dict(g):
    """hparams.stats of the fixture: 'spk 0' and 'spk 1' only, so any other speaker id takes the 'spk 0' fallback."""
    return {f'spk {i}': {'energy': {'mean': float(r[0]), 'std': float(r[1])}, 'pitch': {'mean': float(r[2]), 'std': float(r[3])}}
            for i, r in enumerate(g['cond/speaker_stats'])}


def source_dict(g):
    r = g['cond/source_stats']
    return {'energy': {'mean': float(r[0]), 'std': float(r[1])}, 'pitch': {'mean': float(r[2]), 'std': float(r[3])}}


def stats_rows(g):
    """(B, 4) float64 target statistics per row, 'spk 0' for a speaker without statistics."""
    table = g['cond/speaker_stats']
    return np.stack([table[i] if i < len(table) else table[0] for i in g['cond/speaker_ids'].tolist()]).astype(np.float64)


def symbol_means64(frames_energy, frames_pitch, dur_int, in_lens):
    """extract_features.get_symbols_energy / get_symbols_pitch in float64, padded (B, L) -> two (B, L) arrays."""
    B, L = dur_int.shape
    se, sp = np.zeros((B, L)), np.zeros((B, L))
    for b in range(B):
        idx = 0
        for l in range(int(in_lens[b])):
            d = int(dur_int[b, l])
            if d == 0:
                continue
            se[b, l] = frames_energy[b, idx:idx + d].astype(np.float64).mean()
            voiced = frames_pitch[b, idx:idx + d].astype(np.float64)
            voiced = voiced[voiced > 0.0]
            sp[b, l] = voiced.mean() if voiced.size else 0.0
            idx += d
    return se, sp


def _normalise64(v, tgt_mean, tgt_std, source, alpha):
    zero = v == 0.0
    if source is not None:
        v = (v - source[0]) / source[1] * tgt_std + tgt_mean
    v = (v - tgt_mean) / tgt_std
    v = v * alpha
    return np.where(zero, 0.0, v)


def condition64(energy, pitch, dur_int, in_lens, energy_factors, pitch_factors, stats, source, alpha_energy, alpha_pitch, mode, normalize):
    """dx_prosody_condition in float64: generate.py:165-185, :265-269, model.py:1077-1087, :975-1024.  stats (B, 4) float64, source (4,) or
    None, mode a key of MODES.  -> (energy, pitch) float64 (B, L), zero past in_lens."""
    B, L = energy.shape
    e_out, p_out = np.zeros((B, L)), np.zeros((B, L))
    for b in range(B):
        n = int(in_lens[b])
        e, p = energy[b, :n].astype(np.float64), pitch[b, :n].astype(np.float64)
        e_mean, e_std, p_mean, p_std = (float(x) for x in stats[b])
        if normalize:
            e = _normalise64(e, e_mean, e_std, None if source is None else source[:2], alpha_energy)
            p = _normalise64(p, p_mean, p_std, None if source is None else source[2:], alpha_pitch)
        if energy_factors is not None:
            e = e * energy_factors[b, :n].astype(np.float64)
        if dur_int is not None:
            e = np.where(dur_int[b, :n] == 0, 0.0, e)
            p = np.where(dur_int[b, :n] == 0, 0.0, p)
        voiced = p != 0.0
        if mode == 'add':
            f = pitch_factors[b, :n].astype(np.float64)
            with np.errstate(all='ignore'):
                p = np.where(voiced, (np.log(np.exp(p_std * p + p_mean) + f) - p_mean) / p_std, 0.0)
        elif mode == 'multiply':
            f = pitch_factors[b, :n].astype(np.float64)
            mean = p[voiced].mean() if voiced.any() else 0.0
            p = np.where(voiced, p + (p - mean) * f, 0.0)
        e_out[b, :n], p_out[b, :n] = e, p
    return e_out, p_out


def pcm_rule(audio, lengths=None):
    """generate.py:327 on a float32 array, rows zeroed at and past ``lengths``."""
    audio = np.asarray(audio)
    assert audio.dtype == np.float32
    out = (audio * 32767.5).clip(min=-32768, max=32767).astype(np.int16)
    if lengths is not None:
        for b, n in enumerate(lengths):
            out[b, int(n):] = 0
    return out


def cond_cases(g):
    """Names of the conditioning cases in the fixture: 'src{0,1}_a{1.0,1.3}_{add,multiply}' and 'inference_{add,multiply}'."""
    return [str(n) for n in g['cond/cases']]


def cond_case_args(g, name):
    """-> dict of the arguments of one conditioning case (inputs as stored, float32 / int64)."""
    inference = name.startswith('inference_')
    mode = name.rsplit('_', 1)[1]
    if inference:
        return dict(energy=g['cond/norm_energy'], pitch=g['cond/norm_pitch'], source=None, alpha=1.0, mode=mode, normalize=False,
                    pitch_factors=g[f'cond/pitch_factors_{mode}'])
    src, alpha = name.split('_')[0] == 'src1', float(name.split('_')[1][1:])
    return dict(energy=g['cond/energy'], pitch=g['cond/pitch'], source=g['cond/source_stats'].astype(np.float64) if src else None, alpha=alpha,
                mode=mode, normalize=True, pitch_factors=g[f'cond/pitch_factors_{mode}'])


def within_bar(got, f64, spread):
    """The project's parity bar: max <= 4 x the reference's own fp32 spread + 1e-6, mean <= 2 x its mean spread + 1e-7."""
    d = np.abs(np.asarray(got, dtype=np.float64) - f64)
    return d.max() <= 4 * spread[0] + 1e-6 and d.mean() <= 2 * spread[1] + 1e-7, d.max(), d.mean()
