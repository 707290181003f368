"""Prosody-transfer synthesis on the device: reference prosody -> 16-bit PCM (reference generate.py:188-330,
``generate_batch_mel_specs``).

``symbol_prosody``              frames -> per-symbol energy / voiced-pitch means (extract_features.py:287-342), one launch per batch
``condition_external_prosody``  generate.py:213-278: host durations, speaker statistics with the 'spk 0' fallback, then the
                                zero-preserving source -> target z-score map and the alpha scaling in one launch
``SpeechSynthesizer``           the whole call: host durations, one conditioning launch (which also does ``model.inference``'s own
                                pre-processing, model.py:1077-1087), ``GraphedSynthesizer``'s bucketed graph replay, the batched
                                vocoder on the still-resident mel, and the PCM rule of generate.py:327 on the device

The kernels are csrc/dx_prosody.hip; there is no CPU path.
"""
from __future__ import annotations

import torch

from ._lib import lib
from .durations import get_int_durations
from .inference import GraphedSynthesizer
from .griffin_lim import GriffinLimVocoder
from .vocoder import HOP, HiFiGanVocoder, VocoderStream

PITCH_MODES = {None: 0, 'add': 1, 'multiply': 2}
PROSODY_KEYS = ('duration_preds', 'energy_preds', 'pitch_preds')      # model.inference's external_prosody (already normalised)


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _require_gpu(t, what):
    if t.device.type != 'cuda':
        raise RuntimeError(f'{what} runs on the GPU (gfx950 HIP kernel); there is no CPU path')


def _f32(t, dev):
    return torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()


# ---- frames -> symbols ---------------------------------------------------------------------------------------------------------------
def symbol_prosody(frames_energy, frames_pitch, durations_int, input_lengths):
    """frames_energy, frames_pitch (B, T) fp32 on the device, durations_int (B, L) integers, input_lengths (B,) -> (sym_energy,
    sym_pitch), both (B, L) fp32: extract_features.get_symbols_energy / get_symbols_pitch for every row (energy: mean over the symbol's
    frames; pitch: mean over its frames > 0, 0 if none; 0 for a symbol of no frames and past input_lengths).  A row whose durations sum
    past T raises ValueError (checked on the host copy of the durations, before the launch)."""
    _require_gpu(frames_energy, 'symbol_prosody')
    dev = frames_energy.device
    if frames_energy.dim() != 2 or frames_pitch.shape != frames_energy.shape:
        raise ValueError(f'symbol_prosody: frames_energy {tuple(frames_energy.shape)} and frames_pitch {tuple(frames_pitch.shape)} must be the same (B, T)')
    durations_int = torch.as_tensor(durations_int)
    input_lengths = torch.as_tensor(input_lengths)
    B, T = frames_energy.shape
    if durations_int.dim() != 2 or durations_int.shape[0] != B or input_lengths.shape != (B,):
        raise ValueError(f'symbol_prosody: durations_int {tuple(durations_int.shape)} / input_lengths {tuple(input_lengths.shape)} do not fit a batch of {B}')
    L = durations_int.shape[1]
    host_d, host_n = durations_int.to('cpu', torch.long), input_lengths.to('cpu', torch.long)
    if (host_d < 0).any() or (host_n < 0).any() or (host_n > L).any():
        raise ValueError('symbol_prosody: negative duration, or an input length outside [0, L]')
    totals = (host_d * (torch.arange(L)[None, :] < host_n[:, None])).sum(dim=1).tolist()
    for b, total in enumerate(totals):
        if total > T:
            raise ValueError(f'symbol_prosody: row {b}: durations sum to {total} frames, the batch has {T}')
    fe, fp = _f32(frames_energy, dev), _f32(frames_pitch, dev)
    dur = durations_int.to(device=dev, dtype=torch.long).contiguous()
    lens = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
    se = torch.empty(B, L, dtype=torch.float32, device=dev)
    sp = torch.empty(B, L, dtype=torch.float32, device=dev)
    lib().dx_symbol_prosody(fe.data_ptr(), fp.data_ptr(), T, dur.data_ptr(), lens.data_ptr(), se.data_ptr(), sp.data_ptr(), B, T, L, _stream(dev))
    return se, sp


# ---- conditioning --------------------------------------------------------------------------------------------------------------------
def speaker_stats_table(speaker_ids, hparams):
    """generate.py:242-253: (B, 4) fp32 host table {energy mean, energy std, pitch mean, pitch std} of each row's target speaker, 'spk 0'
    standing in for a speaker without statistics.  KeyError / ValueError as the reference raises them."""
    ids = [int(i) for i in (speaker_ids.tolist() if torch.is_tensor(speaker_ids) else speaker_ids)]
    rows = []
    for speaker_id in ids:
        spk_key = f'spk {speaker_id}'
        if spk_key not in hparams.stats and 'spk 0' in hparams.stats:
            spk_key = 'spk 0'
        if spk_key not in hparams.stats:
            raise KeyError(f"Speaker stats missing for 'spk {speaker_id}' and fallback 'spk 0' not in hparams.stats (keys: {list(hparams.stats.keys())})")
        st = hparams.stats[spk_key]
        row = [st['energy']['mean'], st['energy']['std'], st['pitch']['mean'], st['pitch']['std']]
        if row[1] == 0 or row[3] == 0:
            raise ValueError(f'Speaker stats not initialized for speaker ID {speaker_id}.')
        rows.append(row)
    return torch.tensor(rows, dtype=torch.float32)


def pitch_stats_table(speaker_ids, hparams):
    """model.py:983-985 (``pitch_shift``): each row's own 'spk <id>' pitch statistics, no fallback; the energy columns are unused."""
    ids = [int(i) for i in (speaker_ids.tolist() if torch.is_tensor(speaker_ids) else speaker_ids)]
    return torch.tensor([[0.0, 1.0, hparams.stats[f'spk {i}']['pitch']['mean'], hparams.stats[f'spk {i}']['pitch']['std']] for i in ids],
                        dtype=torch.float32)


def source_stats_row(source_stats):
    """generate.py:254-255, :172-173: (4,) fp32 host row of the source speaker, or None."""
    if source_stats is None:
        return None
    row = [source_stats['energy']['mean'], source_stats['energy']['std'], source_stats['pitch']['mean'], source_stats['pitch']['std']]
    if row[1] == 0 or row[3] == 0:
        raise ValueError('Source stats std cannot be 0.')
    return torch.tensor(row, dtype=torch.float32)


def host_durations(frames, alpha_dur, hparams):
    """generate.py:226-236 for one utterance, in the reference's own float32 torch operations: frame durations -> (seconds, integer frames)
    after the variance exaggeration around the mean of the non-zero durations."""
    frames = torch.as_tensor(frames).detach().to('cpu', torch.float32).clone()
    hop_in_seconds = hparams.hop_length / hparams.sampling_rate
    dur_mask = (frames > 0)
    if dur_mask.any() and alpha_dur != 1.0:
        dur_mean = frames[dur_mask].mean()
        frames[dur_mask] = dur_mean + alpha_dur * (frames[dur_mask] - dur_mean)
        frames = torch.clamp(frames, min=0.0)
    return frames * hop_in_seconds, torch.round(frames).long()


def _raw_prosody(raw, device):
    """entries (generate.py's list of {'durations_frames', 'energy', 'pitch'} per utterance) or padded tensors {'durations_frames',
    'energy', 'pitch', 'input_lengths'} -> (per-row host durations, energy (B, L), pitch (B, L) on the device, host lengths)."""
    if isinstance(raw, dict):
        lens = [int(n) for n in torch.as_tensor(raw['input_lengths']).tolist()]
        frames = torch.as_tensor(raw['durations_frames']).detach().to('cpu')
        if frames.dim() != 2 or len(lens) != frames.shape[0] or any(n < 0 or n > frames.shape[1] for n in lens):
            raise ValueError('external prosody tensors: durations_frames must be (B, L) and input_lengths (B,) within [0, L]')
        rows = [frames[b, :n] for b, n in enumerate(lens)]
        energy, pitch = _f32(raw['energy'], device), _f32(raw['pitch'], device)
        if energy.shape != frames.shape or pitch.shape != frames.shape:
            raise ValueError('external prosody tensors: energy and pitch must have the shape of durations_frames')
        return rows, energy, pitch, lens
    rows = [torch.as_tensor(entry['durations_frames'], dtype=torch.float32) for entry in raw]
    lens = [int(r.numel()) for r in rows]
    L = max(lens)
    energy, pitch = torch.zeros(len(rows), L), torch.zeros(len(rows), L)
    for b, entry in enumerate(raw):
        if len(entry['energy']) != lens[b] or len(entry['pitch']) != lens[b]:
            raise ValueError(f'external prosody entry {b}: durations_frames, energy and pitch differ in length')
        energy[b, :lens[b]] = torch.as_tensor(entry['energy'], dtype=torch.float32)
        pitch[b, :lens[b]] = torch.as_tensor(entry['pitch'], dtype=torch.float32)
    return rows, energy.to(device), pitch.to(device), lens


def _condition(energy, pitch, dur_int, in_lens_i32, energy_factors, pitch_factors, stats, source, alpha_energy, alpha_pitch, mode, normalize):
    """One dx_prosody_condition launch; ``stats`` / ``source`` are host tables (or None).  The inputs are left as they are."""
    _require_gpu(energy, 'prosody conditioning')
    dev = energy.device
    B, L = energy.shape
    ptr = lambda t: None if t is None else t.data_ptr()
    stats = None if stats is None else stats.to(dev)
    source = None if source is None else source.to(dev)
    e_out, p_out = torch.empty_like(energy), torch.empty_like(pitch)
    lib().dx_prosody_condition(energy.data_ptr(), pitch.data_ptr(), ptr(dur_int), in_lens_i32.data_ptr(), ptr(energy_factors), ptr(pitch_factors),
                               ptr(stats), ptr(source), int(source is not None), float(alpha_energy), float(alpha_pitch), int(mode),
                               int(normalize), e_out.data_ptr(), p_out.data_ptr(), B, L, _stream(dev))
    return e_out, p_out


def condition_external_prosody(entries_or_tensors, speaker_ids, hparams, source_stats=None, alpha_dur=1.0, alpha_pitch=1.0, alpha_energy=1.0,
                               device='cuda'):
    """generate.py:213-278: raw per-symbol prosody of a reference utterance (entries or padded tensors, see ``_raw_prosody``) -> the
    ``external_prosody`` dict ``model.inference`` takes ('duration_preds', 'durations_int', 'energy_preds', 'pitch_preds', on the device).
    Durations stay on the host (float32 torch operations as the reference writes them); energy and pitch are mapped from the source
    speaker's statistics into each row's target speaker's, z-scored, zeros preserved, and scaled by alpha in one launch."""
    stats = speaker_stats_table(speaker_ids, hparams)
    source = source_stats_row(source_stats)
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('condition_external_prosody runs on the GPU (gfx950 HIP kernel); there is no CPU path')
    rows, energy, pitch, lens = _raw_prosody(entries_or_tensors, device)
    B, L = energy.shape
    if stats.shape[0] != B:
        raise ValueError(f'condition_external_prosody: {stats.shape[0]} speaker ids for a batch of {B}')
    ext_duration, ext_duration_int = torch.zeros(B, L), torch.zeros(B, L, dtype=torch.long)
    for b, frames in enumerate(rows):
        ext_duration[b, :lens[b]], ext_duration_int[b, :lens[b]] = host_durations(frames, alpha_dur, hparams)
    in_lens = torch.tensor(lens, dtype=torch.int32).to(device)
    e_out, p_out = _condition(energy, pitch, None, in_lens, None, None, stats, source, alpha_energy, alpha_pitch, 0, 1)
    return {'duration_preds': ext_duration.to(device), 'durations_int': ext_duration_int.to(device), 'energy_preds': e_out, 'pitch_preds': p_out}


# ---- PCM -----------------------------------------------------------------------------------------------------------------------------
def to_pcm16(audio, sample_lengths):
    """audio (B, S) fp32 on the device, sample_lengths (B,) -> (B, S) int16: ``(audio * 32767.5).clip(-32768, 32767).astype(int16)``
    (generate.py:327), 0 at and past each row's length."""
    _require_gpu(audio, 'to_pcm16')
    if audio.dim() != 2:
        raise ValueError(f'to_pcm16: audio must be (B, S), got {tuple(audio.shape)}')
    dev = audio.device
    audio = audio.float().contiguous()
    B, S = audio.shape
    lens = torch.as_tensor(sample_lengths).to(device=dev, dtype=torch.int32).contiguous()
    if lens.shape != (B,):
        raise ValueError(f'to_pcm16: {tuple(lens.shape)} sample lengths for a batch of {B}')
    out = torch.empty(B, S, dtype=torch.int16, device=dev)
    lib().dx_pcm16(audio.data_ptr(), lens.data_ptr(), out.data_ptr(), B, S, _stream(dev))
    return out


class _PcmChunks:
    """``SpeechSynthesizer.stream``'s 'chunks': a ``VocoderStream`` whose steps also carry the chunk as 16-bit PCM."""

    def __init__(self, vocoder, mel, lengths, chunk_frames, pcm16, use_graph):
        self.pcm = None
        tail = None
        if pcm16 and use_graph:                                   # dx_pcm16 as the captured chunk's last launch but one, into a buffer of its own
            B, S = mel.shape[0], int(chunk_frames) * HOP
            self.pcm = torch.zeros(B, max(S, 1), dtype=torch.int16, device=mel.device)
            full = torch.full((B,), S, dtype=torch.int32, device=mel.device)       # the chunk is already 0 past each row's end
            tail = lambda audio: lib().dx_pcm16(audio.data_ptr(), full.data_ptr(), self.pcm.data_ptr(), B, S, _stream(audio.device))
        self.pcm16 = pcm16
        self.voc = VocoderStream(vocoder, mel, lengths, chunk_frames, use_graph, clone=True, tail=tail)

    def __len__(self):
        return len(self.voc)

    def __iter__(self):
        return self

    def __next__(self):
        audio, valid = next(self.voc)
        if not self.pcm16:
            return None, audio, valid
        return (self.pcm.clone() if self.pcm is not None else to_pcm16(audio, valid)), audio, valid


# ---- the whole call ------------------------------------------------------------------------------------------------------------------
class SpeechSynthesizer:
    """``generate_batch_mel_specs`` from the collated batch to PCM, device-resident: ``model`` a ``DaftExprt``, ``vocoder`` a
    ``HiFiGanVocoder``, or a ``GriffinLimVocoder`` where no checkpoint is at hand (its audio has 256 T + 512 samples per row, and it cannot
    ``stream``).  The acoustic model runs through a ``GraphedSynthesizer`` (``self.synth``: one captured graph per
    (B, L up to 16, T up to 64) bucket)."""

    def __init__(self, model, hparams, vocoder, max_graphs=32):
        self.synth = GraphedSynthesizer(model, hparams, max_graphs)
        self.hparams = hparams
        self.vocoder = vocoder

    def prepare(self, inputs, pitch_transform, external_prosody, source_stats=None, alpha_dur=1.0, alpha_pitch=1.0, alpha_energy=1.0):
        """The prosody stage of ``GraphedSynthesizer.prepare`` with ONE launch in place of the ATen chain.  ``external_prosody``: either
        ``model.inference``'s dict (already normalised: only factors, zeroing and the pitch transform apply, and the alphas and
        source_stats must be left at their defaults) or raw reference prosody as ``condition_external_prosody`` takes it."""
        symbols, dur_factors, energy_factors, pitch_factors, input_lengths, speaker_ids = inputs
        _require_gpu(symbols, 'SpeechSynthesizer')
        if pitch_transform not in ('add', 'multiply'):
            raise NotImplementedError
        dev, hp = symbols.device, self.hparams
        B, L = symbols.shape
        normalised = isinstance(external_prosody, dict) and all(k in external_prosody for k in PROSODY_KEYS)
        if normalised:
            if source_stats is not None or (alpha_dur, alpha_pitch, alpha_energy) != (1.0, 1.0, 1.0):
                raise ValueError('source_stats and the alphas apply to raw reference prosody, not to already normalised external_prosody')
            duration_preds = external_prosody['duration_preds']
            energy, pitch = _f32(external_prosody['energy_preds'], dev), _f32(external_prosody['pitch_preds'], dev)
            stats = pitch_stats_table(speaker_ids, hp) if pitch_transform == 'add' else None
            source = None
        else:
            stats, source = speaker_stats_table(speaker_ids, hp), source_stats_row(source_stats)
            rows, energy, pitch, lens = _raw_prosody(external_prosody, dev)
            if energy.shape != (B, L) or lens != [int(n) for n in input_lengths.tolist()]:
                raise ValueError('external prosody does not match the symbols: shape or lengths differ')
            duration_preds = torch.zeros(B, L)
            for b, frames in enumerate(rows):
                duration_preds[b, :lens[b]] = host_durations(frames, alpha_dur, hp)[0]
            duration_preds = duration_preds.to(dev)
        dur, dur_int, totals = get_int_durations(duration_preds * dur_factors, hp, return_totals=True)      # host library, bit-exact
        energy_out, pitch_out = _condition(energy, pitch, dur_int.contiguous(), input_lengths.to(torch.int32), _f32(energy_factors, dev),
                                           _f32(pitch_factors, dev), stats, source, alpha_energy, alpha_pitch,
                                           PITCH_MODES[pitch_transform], 0 if normalised else 1)
        return dict(symbols=symbols, in_lens=input_lengths, dur=dur, dur_int=dur_int, energy=energy_out, pitch=pitch_out,
                    out_host=[max(1, t) for t in totals], n_frames=max(totals))

    def __call__(self, inputs, pitch_transform, external_prosody, external_embeddings, external_accent_emb, source_stats=None,
                 alpha_dur=1.0, alpha_pitch=1.0, alpha_energy=1.0, pcm16=True, use_graph=True):
        """``DaftExprt.inference``'s arguments (+ raw prosody, see ``prepare``) -> dict: 'pcm' (B, 256 T_max) int16 on the device (None
        with ``pcm16=False``), 'audio' fp32, 'sample_lengths', 'mel', 'output_lengths', 'encoder_preds', 'weights'.  The mel goes from
        the acoustic model to the vocoder on the device."""
        prep = self.prepare(inputs, pitch_transform, external_prosody, source_stats, alpha_dur, alpha_pitch, alpha_energy)
        encoder_preds, (mel, out_lens), weights = self.synth.run(prep, external_embeddings, external_accent_emb, use_graph)
        with torch.no_grad():
            audio, voc_lengths = self.vocoder.infer_batch(mel, prep['out_host'])
            if isinstance(self.vocoder, HiFiGanVocoder):
                sample_lengths = out_lens * HOP
            else:                                                 # any other vocoder states its own lengths (Griffin-Lim: 256 T + 512)
                sample_lengths = torch.as_tensor(voc_lengths).to(device=audio.device, dtype=torch.long)
            pcm = to_pcm16(audio, sample_lengths) if pcm16 else None
        return dict(pcm=pcm, audio=audio, sample_lengths=sample_lengths, mel=mel, output_lengths=out_lens, encoder_preds=encoder_preds,
                    weights=weights)

    def stream(self, inputs, pitch_transform, external_prosody, external_embeddings, external_accent_emb, source_stats=None,
               alpha_dur=1.0, alpha_pitch=1.0, alpha_energy=1.0, pcm16=True, use_graph=True, chunk_frames=32):
        """``__call__`` with the audio delivered in chunks of ``chunk_frames`` mel frames: the same dict, with 'pcm' and 'audio' replaced by
        'chunks', an iterator (with a length) of (pcm (B, 256 chunk_frames) int16 or None, audio fp32, valid (B,) samples of the chunk that
        belong to each row).  The acoustic model runs whole, as in ``__call__`` (it is not autoregressive); the vocoder is
        ``HiFiGanVocoder.stream``, so the chunks concatenated are bitwise ``__call__``'s 'audio' and 'pcm'.  With ``use_graph`` the PCM
        conversion is one more launch of the captured chunk (samples past a row's end are already 0 there).  A ``GriffinLimVocoder``
        cannot stream (every iteration reads the whole row: the algorithm is not causal) and raises NotImplementedError."""
        if isinstance(self.vocoder, GriffinLimVocoder):
            raise NotImplementedError('SpeechSynthesizer.stream: Griffin-Lim is not causal (every iteration reads the whole utterance); use __call__')
        prep = self.prepare(inputs, pitch_transform, external_prosody, source_stats, alpha_dur, alpha_pitch, alpha_energy)
        encoder_preds, (mel, out_lens), weights = self.synth.run(prep, external_embeddings, external_accent_emb, use_graph)
        chunks = _PcmChunks(self.vocoder, mel, prep['out_host'], chunk_frames, pcm16, use_graph)
        return dict(chunks=chunks, sample_lengths=out_lens * HOP, mel=mel, output_lengths=out_lens, encoder_preds=encoder_preds,
                    weights=weights)

    def from_reference_audio(self, wavs, wav_lengths, frames_pitch, durations_int, inputs, pitch_transform, external_embeddings,
                             external_accent_emb, **kwargs):
        """Prosody taken from reference recordings: wavs (B, S) on the device with their sample lengths, their frame pitch (B, >= T) and
        the integer symbol durations (B, L) of their alignment.  Frame energy comes from the mel front end, symbol means from
        ``symbol_prosody``, then the call above with the raw prosody (``kwargs``: source_stats, alphas, pcm16, use_graph)."""
        from .mel import MelSpectrogram
        if getattr(self, '_mel', None) is None or self._mel.device != wavs.device:
            self._mel = MelSpectrogram(self.hparams, device=wavs.device)
        _, energy, _ = self._mel(wavs, wav_lengths)
        T = energy.shape[1]
        if frames_pitch.shape[1] < T:
            raise ValueError(f'frames_pitch has {frames_pitch.shape[1]} frames, the recordings have {T}')
        input_lengths = inputs[4]
        sym_energy, sym_pitch = symbol_prosody(energy, frames_pitch[:, :T].to(energy.device), durations_int, input_lengths)
        raw = {'durations_frames': torch.as_tensor(durations_int).to('cpu', torch.float32), 'energy': sym_energy, 'pitch': sym_pitch,
               'input_lengths': input_lengths}
        return self(inputs, pitch_transform, raw, external_embeddings, external_accent_emb, **kwargs)
