"""hipGraph-captured inference forward (BASELINE.json config 4).

``DaftExprt.inference`` (reference model.py:1026-1114) interleaves host work (``get_int_durations``: double-precision
Python, ``.item()`` loops; ``int(torch.max(...))``; asserts) with device work, which blocks graph capture.
Here the host part runs FIRST (durations -> integer frames, lengths, T_max, all bit-exact and on the CPU), then the whole
device part -- speaker projection, FiLM generation, phoneme encoder, Gaussian upsampler, frame decoder -- is ONE captured HIP
graph per shape BUCKET, replayed with new inputs copied into its static buffers.

Length bucketing.  A graph is keyed by (B, L_max rounded up to 16, T_max rounded up to 64), not by the exact padded shape: every
new T_max would otherwise re-capture.  The reference's results depend on the padded length (the k = 3 convolutions see zero
padding at the end of the (B, N_max) grid), so the kernels are told separately how many rows EXIST
(``Lengths.exist`` -> the ``rows_exist`` argument of the C ABI: device memory, re-read by every replay) and how many are
allocated (the tensor shape): rows in between are treated exactly like the reference's non-existent ones, and a replay at any
(L_max, T_max) inside the bucket equals the eager forward at that exact shape.

Batched accent encoder.  The reference obtains the accent embedding by running ``model.accent_encoder`` on each reference
recording with B = 1 and averaging (scripts/synthesize.py:420-448).  ``accent_embedding`` runs all recordings as one padded batch
with ``exist = lengths``: every row sees no padding at all, i.e. behaves as if it were run alone, so the batch reproduces the
per-recording results.
"""
from __future__ import annotations

import torch

from . import ops
from .durations import get_int_durations
from .functional import Lengths
from .graphs import Entry, GraphCache, capture, warm_up

L_STEP, T_STEP = 16, 64
PADDED = ('symbols', 'dur', 'dur_int', 'energy', 'pitch')     # ``run``'s static buffers of the bucket's L; every other one has its exact shape


def _up(n, step):
    return (int(n) + step - 1) // step * step


def _stage(static, live, padded):
    """The live tensors into a graph's static buffers.  The ``padded`` ones are longer on the last axis: zeroed, live rows in front."""
    for k, v in live.items():
        if k in padded:
            static[k].zero_()
            static[k][..., :v.shape[-1]].copy_(v)
        else:
            static[k].copy_(v)


class GraphedSynthesizer:
    def __init__(self, model, hparams, max_graphs=32):
        self.model = model.eval()
        self.hparams = hparams
        self.graphs = GraphCache(max_graphs, 'least_used')            # per bucket: one graph, its ``static`` inputs, its ``outs``
        self.accent_graphs = GraphCache(max_graphs, 'least_used')     # ... and its ``out``
        self.max_graphs = max_graphs

    # -- host side: exactly the reference's pre-processing, model.py:1068-1087 --------------------------------------------
    def prepare(self, inputs, pitch_transform, external_prosody):
        symbols, dur_factors, energy_factors, pitch_factors, input_lengths, speaker_ids = inputs
        m = self.model
        duration_preds = external_prosody['duration_preds'] * dur_factors
        duration_preds, durations_int, totals = get_int_durations(duration_preds, self.hparams, return_totals=True)   # host library, C
        energy = external_prosody['energy_preds'] * energy_factors
        pitch = external_prosody['pitch_preds']
        energy[durations_int == 0] = 0.0
        pitch[durations_int == 0] = 0.0
        if pitch_transform == 'add':
            pitch = m.pitch_shift(pitch, pitch_factors, self.hparams, speaker_ids)
        elif pitch_transform == 'multiply':
            pitch = m.pitch_multiply(pitch, pitch_factors)
        else:
            raise NotImplementedError
        out_host = [max(1, t) for t in totals]
        return dict(symbols=symbols, in_lens=input_lengths, dur=duration_preds, dur_int=durations_int,
                    energy=energy, pitch=pitch, out_host=out_host, n_frames=max(totals))

    # -- device side -----------------------------------------------------------------------------------------------------
    def _device_forward(self, st):
        m = self.model
        spk = m.spk_projection(ops.l2_normalize(st['spk_embs']), need_dx=False)
        film = m.style_adapter(st['accent_emb'] + spk)
        in_lens = Lengths(st['in_lens'], host=st['in_host'], i32=st['in_lens_i32'], exist=st.get('in_exist'))
        enc = m.phoneme_encoder(st['symbols'], film['phoneme_encoder'], in_lens)
        x, weights = m.gaussian_upsampling(enc, st['dur'], st['dur_int'], st['energy'], st['pitch'], in_lens, n_frames=st['n_frames'])
        out_lens = Lengths(st['out_lens'], host=st['out_host'], i32=st['out_lens_i32'], exist=st.get('out_exist'))
        mel = m.frame_decoder(x, film['frame_decoder'], out_lens)
        return mel, weights

    def __call__(self, inputs, pitch_transform, external_prosody, external_embeddings, external_accent_emb, use_graph=True):
        """Same arguments as ``DaftExprt.inference``; returns the same triple."""
        return self.run(self.prepare(inputs, pitch_transform, external_prosody), external_embeddings, external_accent_emb, use_graph)

    def run(self, prep, external_embeddings, external_accent_emb, use_graph=True):
        """The device forward for a prosody stage that is already done: ``prep`` is what ``prepare`` returns (``speech.SpeechSynthesizer``
        builds it with one conditioning launch instead).  Returns ``DaftExprt.inference``'s triple."""
        dev = prep['symbols'].device
        out_lens = torch.tensor(prep['out_host'], dtype=torch.long, device=dev)
        B, L = prep['symbols'].shape
        T = prep['n_frames']
        live = dict(symbols=prep['symbols'].contiguous(), dur=prep['dur'].contiguous(), dur_int=prep['dur_int'].contiguous(),
                    energy=prep['energy'].contiguous(), pitch=prep['pitch'].contiguous(), in_lens=prep['in_lens'],
                    in_lens_i32=prep['in_lens'].to(torch.int32), out_lens=out_lens, out_lens_i32=out_lens.to(torch.int32),
                    spk_embs=external_embeddings.contiguous(), accent_emb=external_accent_emb.contiguous())
        with torch.no_grad():
            if not use_graph:
                mel, weights = self._device_forward({**live, 'in_host': prep['in_lens'].tolist(), 'out_host': prep['out_host'], 'n_frames': T})
            else:
                Lb, Tb = _up(L, L_STEP), _up(max(T, 1), T_STEP)
                key = (B, Lb, Tb, self.model.runtime.precision)
                entry = self.graphs.get(key)
                if entry is None:
                    static = {k: (torch.zeros(B, Lb, dtype=v.dtype, device=dev) if k in PADDED else v.clone()) for k, v in live.items()}
                    _stage(static, live, PADDED)
                    static['in_exist'] = torch.full((B,), L, dtype=torch.int32, device=dev)      # rows that EXIST on each axis: re-read by
                    static['out_exist'] = torch.full((B,), T, dtype=torch.int32, device=dev)    # every replay (set per call below)
                    # host-side shape metadata of the BUCKET (lengths as Python ints only size tensors here)
                    forward = lambda: self._device_forward({**static, 'in_host': [Lb] * B, 'out_host': [Tb] * B, 'n_frames': Tb})
                    warm_up(forward)                                      # packs weights, sets kernel attributes
                    graph, outs = capture(forward)
                    entry = self.graphs[key] = Entry([graph], static=static, outs=outs)
                entry.hits += 1
                static, outs = entry.static, entry.outs
                ops.repack_all(self.model.runtime)        # weights changed since capture (load_state_dict, an optimiser step)? one
                                                          # launch rewrites the SAME pack buffers the captured kernels read
                _stage(static, live, PADDED)
                static['in_exist'].fill_(L)
                static['out_exist'].fill_(T)
                entry.graphs[0].replay()
                mel, weights = outs[0][:, :, :T].clone(), outs[1][:, :L, :T].clone()
        encoder_preds = [prep['dur'], prep['dur_int'], prep['energy'], prep['pitch'], prep['in_lens']]
        return encoder_preds, [mel, out_lens], weights

    # -- batched accent encoder ----------------------------------------------------------------------------------------------
    def accent_embeddings(self, frames_energy, frames_pitch, mel_specs, lengths, use_graph=True):
        """(R, T) energy / pitch, (R, n_mel, T) mels and (R,) lengths of R reference recordings, right-zero-padded -> (R, 128): row r
        is what ``model.accent_encoder`` returns for recording r run ALONE (B = 1, no padding), as scripts/synthesize.py:420-448 does."""
        m = self.model
        dev = mel_specs.device
        R, n_mel, T = mel_specs.shape
        lengths = lengths.to(dev)
        host = lengths.tolist()
        i32 = lengths.to(torch.int32)

        def run(e, p, mel, lens_t, lens_i32, host_lens):
            # exist = lengths: rows beyond a recording's own length do not exist, so it behaves as if alone
            return m.accent_encoder(e, p, mel, Lengths(lens_t, host=host_lens, i32=lens_i32, exist=lens_i32))

        with torch.no_grad():
            if not use_graph:
                return run(frames_energy.contiguous(), frames_pitch.contiguous(), mel_specs.contiguous(), lengths, i32, host)
            Tb = _up(T, T_STEP)
            key = (R, Tb, self.model.runtime.precision)
            live = dict(e=frames_energy, p=frames_pitch, mel=mel_specs, lens=lengths, i32=i32)
            entry = self.accent_graphs.get(key)
            if entry is None:
                static = dict(e=torch.zeros(R, Tb, device=dev), p=torch.zeros(R, Tb, device=dev), mel=torch.zeros(R, n_mel, Tb, device=dev),
                              lens=lengths.clone(), i32=i32.clone())
                _stage(static, live, ('e', 'p', 'mel'))
                forward = lambda: run(static['e'], static['p'], static['mel'], static['lens'], static['i32'], [Tb] * R)
                warm_up(forward)
                graph, out = capture(forward)
                entry = self.accent_graphs[key] = Entry([graph], static=static, out=out)
            entry.hits += 1
            ops.repack_all(self.model.runtime)
            _stage(entry.static, live, ('e', 'p', 'mel'))
            entry.graphs[0].replay()
            return entry.out.clone()

    def accent_embedding(self, frames_energy, frames_pitch, mel_specs, lengths, use_graph=True):
        """The averaged accent embedding (1, 128) of scripts/synthesize.py:446-448."""
        return self.accent_embeddings(frames_energy, frames_pitch, mel_specs, lengths, use_graph).mean(dim=0, keepdim=True)

    # -- accent embedding from reference audio -------------------------------------------------------------------------------
    def trimmed_audio_features(self, wavs, wav_lengths, frames_pitch, pitch_lengths):
        """scripts/synthesize.py:424-429 on the device: (R, S) waveforms -> mel and frame energy (``mel.MelSpectrogram`` with this
        synthesizer's hparams), each row trimmed with its pitch to min(pitch_lengths[r], mel frames) and zero after that.
        -> (energy (R, T), pitch (R, T), mels (R, n_mel, T), lengths (R,) int64), T = the longest trimmed row."""
        from .mel import MelSpectrogram
        if getattr(self, '_mel', None) is None or self._mel.device != wavs.device:
            self._mel = MelSpectrogram(self.hparams, device=wavs.device)
        mels, energy, frames = self._mel(wavs, wav_lengths)
        dev = mels.device
        pl = torch.as_tensor(pitch_lengths).to(device=dev, dtype=torch.long)
        lengths = torch.minimum(pl, frames)
        T = max(1, int(lengths.max()))
        if frames_pitch.shape[1] < T:
            raise ValueError(f'frames_pitch has {frames_pitch.shape[1]} frames, pitch_lengths asks for {T}')
        keep = torch.arange(T, device=dev)[None, :] < lengths[:, None]
        energy = energy[:, :T].masked_fill(~keep, 0.0).contiguous()
        pitch = frames_pitch[:, :T].to(dev).float().masked_fill(~keep, 0.0).contiguous()
        mels = mels[:, :, :T].masked_fill(~keep[:, None, :], 0.0).contiguous()
        return energy, pitch, mels, lengths

    def accent_embeddings_from_audio(self, wavs, wav_lengths, frames_pitch, pitch_lengths, use_graph=True):
        """(R, S) reference recordings on the device with their sample lengths, and their frame pitch (R, T_p) with pitch_lengths ->
        (R, 128) accent embeddings: mel and energy computed on the device, trimmed as scripts/synthesize.py:428-429 does, then
        ``accent_embeddings``.  Pitch stays an input (the reference tracks it with REAPER)."""
        energy, pitch, mels, lengths = self.trimmed_audio_features(wavs, wav_lengths, frames_pitch, pitch_lengths)
        return self.accent_embeddings(energy, pitch, mels, lengths, use_graph)

    def accent_embedding_from_audio(self, wavs, wav_lengths, frames_pitch, pitch_lengths, use_graph=True):
        """The averaged accent embedding (1, 128) of scripts/synthesize.py:444-447, from audio."""
        return self.accent_embeddings_from_audio(wavs, wav_lengths, frames_pitch, pitch_lengths, use_graph).mean(dim=0, keepdim=True)
