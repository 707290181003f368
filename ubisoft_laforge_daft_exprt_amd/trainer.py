"""The reference's optimiser-step structure around the HIP path ("boundary only" -- the trainer file itself
never travels, but a drop-in must reproduce what it does between two parameter updates).

One ``Trainer.train_step`` = src/daft_exprt/train.py:390-539 without logging / validation / checkpoint cadence:

    for each of ``accumulation_steps`` micro-batches:                       train.py:390-436
        parse_batch -> keep RAW frame energy / pitch for the consistency losses -> on-device batch conditioning
        -> model forward -> DaftExprtLoss(outputs, targets, iteration) -> (loss / accumulation_steps).backward()
    gradient exchange (bucketed RCCL all-reduce, launched during the LAST micro-batch's backward)        train.py:272 (DDP)
    clip_grad_norm_(parameters, grad_clip_thresh) + Adam(lr(iteration)) as ONE fused launch per bucket  train.py:443-445
    iteration += 1; lr = update_learning_rate(hparams, iteration)                                        train.py:517-539

MI355X-specific structure of one update (``use_graphs=True``, the default):
  * the backward runs in PHASES, cut where a finished part's gradient buckets can be handed to RCCL while the rest still computes
    (``cuts``; functional.cut): A = zero the gradient buckets, forward, loss, backward of everything downstream of the accent
    embedding (29 MB of gradients); B = backward of the accent encoder's four FFT blocks (13.7 MB); C = prenet layers 2 and 1
    (14.2 MB, 12.6 of them the 1024 x 1024 layer); D = prenet layer 0 (1 MB).  Each phase ends by launching its queued weight
    gradients (ops.flush_wgrads) and then its group's bucketed all-reduces on RCCL's stream: group g travels under phase g + 1, and
    only group D's 1 MB (2 % of the 57.5 MB) is launched after the last backward kernel (``exchange_plan()``).  With ONE rank there
    is nothing to exchange and the step is one phase (``cuts='auto'``).
  * the device work of each phase is ONE captured HIP graph per padded batch shape, replayed with the new batch copied into the
    static input buffers: ~600 kernel launches cost the host 7 ms per step when issued one by one from Python -- as much as the GPU
    needs to execute them -- and ~20 us per graph launch.  The same phase order runs eagerly (``use_graphs=False``).
  * what changes between replays lives in device memory the graphs read: the batch, the lengths, the adversarial-loss weight, the
    conditioner's speaker tables (updated in place, conditioning.BatchConditioner) and a dropout seed offset that the first graph
    increments (``runtime.seed_offset``), so every replay draws fresh dropout masks.  The MFMA weight packs are re-packed by the
    optimiser step, and at the top of ``train_step`` when anything else changed the parameters (``load_checkpoint``).
  * the optimiser (fused Adam, LR by value) and the one-launch weight re-pack stay outside the graphs: ten launches.
  * ``validate`` = train.py:163-209: eval-mode forward + loss under ``no_grad`` as one captured graph per padded shape.
  * ``bucket=(l_step, t_step)``: the reference's collate pads every batch to its own longest utterance, so the exact padded shape
    changes almost every step and every new shape costs an eager step plus a capture.  In bucketed mode a micro-batch whose longest
    utterances are (L, T) runs at (L rounded up to l_step, T rounded up to t_step): the padded inputs get zero tails, and device
    int32 vectors ``exist`` = L / T (functional.Lengths.exist, in the batch's length slots: pad_batch) tell every k = 3 launch,
    forward and backward, that rows beyond them do not exist.  With dropout off the step computes what the exact-shape step
    computes ("logical rows vs stride"); dropout masks are drawn over the bucket's row stride instead.

fp16 operand mode (no reference counterpart: the reference trains in fp32): gradients that live in 16-bit tensors would underflow, so the
backward runs on loss * scale and the fused Adam multiplies by 1 / scale.  A non-finite gradient norm SKIPS the update -- parameters and
both moments untouched -- where the reference steps anyway (train.py:443-450); that is the one deliberate deviation.  Two modes:
  * static (the default): ``hparams.loss_scale`` (4096) for the whole run, a host value in the launch arguments.  ``skipped_steps()``
    counts the skipped updates (a host sync); nothing lowers the scale, and the bias-correction step counts skipped updates too.
  * dynamic (``hparams.dynamic_loss_scale = True``; active only when the model runs in fp16, inert in every other precision): the
    scale is a power of two in device memory (optim.LossScaler) with torch.amp.GradScaler's rules -- halved (``loss_scale_backoff``)
    on a skipped update, doubled (``loss_scale_growth``) after ``loss_scale_growth_interval`` applied ones in a row, kept within
    [``loss_scale_min``, ``loss_scale_max``].  The captured graphs read it through a pointer and the optimiser's launch sequence
    (norm, decision, Adam) updates it: no host sync, no re-capture when it changes.  The bias-correction step is the number of
    APPLIED updates.  ``iteration`` -- and with it the LR schedule and the adversarial warm-up -- advances on a skipped update too,
    as it does when a GradScaler is used with a scheduler.  ``scaler_state()`` reports it, ``checkpoint()`` stores it (``loss_scaler``).

Like the reference, a NaN loss does not stop the update (train.py:445-450 only skips LOGGING); ``nan_steps`` counts them.
The iteration counter starts at 1 (train.py:286) and the learning rate of step ``i`` is ``update_learning_rate(hparams, i)``.
``save_checkpoint`` / ``load_checkpoint`` use the reference's dict layout (train.py:63-145) including the torch.optim.Adam
optimiser layout.
"""
from __future__ import annotations

import math
import os

import torch

from . import ops
from .ddp import GradientReducer
from .functional import Lengths
from .graphs import Entry, GraphCache, capture, warm_up
from .loss import LossTerms
from .hparams import loss_scale_config
from .optim import FusedAdam, LossScaler, update_learning_rate


def group_of(name: str, levels: int = 3) -> int:
    """Gradient-exchange group of a parameter = the backward PHASE after which its gradient is complete (``levels`` cuts, functional.cut):
    0 = everything downstream of the accent embedding, 1 = the accent encoder's four FFT blocks, 2 = prenet layers 1 and 2,
    3 = prenet layer 0 and the accent encoder's prosody embeddings (their gradients are complete earlier; they ride in the last, 1 MB
    group so that every group is ONE contiguous run of the reversed registration order)."""
    if levels < 1 or not name.startswith('accent_encoder.'):
        return 0
    if name.startswith('accent_encoder.blocks.'):
        return 1
    if name.startswith(('accent_encoder.convs.0.', 'accent_encoder.convs.2.', 'accent_encoder.energy_embedding.', 'accent_encoder.pitch_embedding.')):
        return min(levels, 3)
    return min(levels, 2)


def pad_batch(inputs, Lb, Tb):
    """A parsed micro-batch (DaftExprt.parse_batch) whose longest utterances are (L, T), padded with zeros to (Lb >= L, Tb >= T) rows:
    -> (inputs, targets) of the padded shape.  Its length slots hold ``Lengths`` with ``exist`` (device int32 [B]) = L / T: rows beyond
    them do not exist for the k = 3 launches; and with the PADDED shape's host lengths (host metadata only sizes tensors, so a graph
    captured on one batch serves every batch of its bucket)."""
    B, L = inputs[0].shape
    T = inputs[8].shape[2]
    if Lb < L or Tb < T:
        raise ValueError(f'cannot pad a ({L}, {T}) batch to ({Lb}, {Tb})')
    pad = lambda t, n: torch.nn.functional.pad(t, (0, n - t.shape[-1])) if t.shape[-1] != n else t
    padded = list(inputs)
    for i in (0, 1, 2, 3, 4):                         # symbols, durations (float, int), symbol energy / pitch: (B, L)
        padded[i] = pad(inputs[i], Lb)
    for i in (6, 7, 8):                               # frame energy / pitch (B, T), mels (B, n_mel, T)
        padded[i] = pad(inputs[i], Tb)
    for i, n, e in ((5, Lb, L), (9, Tb, T)):
        padded[i] = Lengths(inputs[i], host=[n] * B, exist=torch.full((B,), e, dtype=torch.int32, device=inputs[i].device))
    return _with_targets(tuple(padded))


def _with_targets(inputs):
    return inputs, (inputs[1], inputs[3], inputs[4], inputs[8], inputs[9], inputs[10])      # the targets alias the inputs, as parse_batch builds them


PHASE_NAMES = ('A: forward, loss, backward of decoder / upsampler / phoneme encoder / style adapter / classifier',
               'B: backward of the accent encoder\'s four FFT blocks', 'C: backward of prenet layers 2 and 1 (+ prosody embeddings)',
               'D: backward of prenet layer 0')


class Trainer:
    def __init__(self, model, criterion, hparams, conditioner=None, process_group=None, bucket_mb=16.0, grad_sink=True,
                 use_graphs=True, max_graphs=16, cuts='auto', bucket=None):
        """``cuts``: how many times the backward is cut into phases (0..3) so that a finished phase's gradient buckets are exchanged
        while the next phase computes.  'auto' = 3 when there is more than one rank, 0 (one phase, one graph) otherwise.
        ``bucket``: None (graphs keyed on each micro-batch's exact padded shape) or (l_step, t_step), e.g. (inference.L_STEP,
        inference.T_STEP) = (16, 64): micro-batches are padded up to multiples of these and one graph serves every batch of a bucket."""
        self.model, self.criterion, self.hparams, self.conditioner = model, criterion, hparams, conditioner
        self.device = next(model.parameters()).device
        import torch.distributed as dist
        world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.cut_levels = (3 if (world > 1 or os.environ.get('DX_FORCE_COLLECTIVES', '0') == '1') else 0) if cuts == 'auto' else int(cuts)
        if not 0 <= self.cut_levels <= 3:
            raise ValueError(f'cuts must be 0..3 or "auto", got {cuts!r}')
        self.reducer = GradientReducer(model, bucket_mb=bucket_mb, process_group=process_group, grad_sink=grad_sink,
                                       group_of=lambda n: group_of(n, self.cut_levels), explicit_launch=True)
        self.use_graphs, self.max_graphs = bool(use_graphs), int(max_graphs)
        if bucket is not None:
            bucket = (int(bucket[0]), int(bucket[1]))
            if bucket[0] < 1 or bucket[1] < 1:
                raise ValueError(f'bucket steps must be positive, got {bucket!r}')
        self.bucket = bucket
        # the FFT blocks' weight gradients go straight into the buckets (sink) and have no consumer before the exchange, so they are
        # queued during backward and launched 8 layers at a time (ops.flush_wgrads, after every backward phase below)
        model.runtime.defer_wgrad = bool(grad_sink)
        # fp16 operand mode: gradients that live in 16-bit tensors (dqkv, the 1024-wide hidden gradients) would underflow; the
        # backward runs on loss * loss_scale and the fused Adam multiplies by 1 / loss_scale (static scale; bf16 needs none).
        # An overflow (non-finite gradient norm) SKIPS the update on every rank (the norm is computed after the all-reduce, so all
        # ranks see the same value): ``skipped_steps()`` counts them, ``hparams.loss_scale`` lowers the scale.
        # ``hparams.dynamic_loss_scale``: the scale lives on the device and follows GradScaler's rules (module docstring); only in fp16.
        scale_cfg = loss_scale_config(hparams)
        self._fp16_loss_scale = scale_cfg['loss_scale']
        self.scaler = LossScaler(scale_cfg, self.device) if scale_cfg['dynamic'] and model.runtime.precision == 'fp16' else None
        self.graphs = GraphCache(self.max_graphs, 'least_used')      # per padded shape: one graph per backward phase, static ``inputs``,
        self.val_graphs = GraphCache(self.max_graphs, 'oldest')      # captured ``loss`` and ``terms_dev``
        self._conditioner_generation = getattr(conditioner, 'generation', None)
        self.adv_weight = torch.zeros((), dtype=torch.float32, device=self.device)    # read by the captured loss
        self.val_adv_weight = torch.zeros((), dtype=torch.float32, device=self.device)   # validation: iteration = 0 (train.py:198)
        self._one = torch.ones((), dtype=torch.float32, device=self.device)
        if model.runtime.seed_offset is None:
            model.runtime.seed_offset = torch.zeros((), dtype=torch.int64, device=self.device)
        self.optimizer = FusedAdam(self.reducer, lr=hparams.initial_learning_rate, betas=hparams.betas, eps=hparams.epsilon,
                                   weight_decay=hparams.weight_decay, grad_clip_thresh=hparams.grad_clip_thresh, scaler=self.scaler)
        self.accumulation_steps = int(getattr(hparams, 'accumulation_steps', 1))
        self.iteration = 1
        self.learning_rate = update_learning_rate(hparams, self.iteration)
        self.last_learning_rate = self.learning_rate      # the rate the most recent update used (what a checkpoint records, train.py:451-455)
        self.nan_steps = 0
        self.best_val_loss = float('inf')
        model.train()

    @property
    def loss_scale(self):
        """The scale the next backward runs on (dynamic mode: its current value, one host transfer); 1 outside fp16."""
        if self.scaler is not None:
            return self.scaler.state()['scale']
        return self._fp16_loss_scale if self.model.runtime.precision == 'fp16' else 1.0

    def skipped_steps(self) -> int:
        """Updates the fused Adam skipped because the gradient norm was not finite (one host sync)."""
        return self.optimizer.skipped_steps()

    def scaler_state(self):
        """``{scale, applied, good_steps, skipped}``: the scale of the next backward, the updates applied so far (the bias-correction
        step), the applied updates in a row since the scale last changed, the updates skipped so far.  Dynamic mode: a snapshot of the
        device state taken now, fetched with a single transfer on first access (optim.ScalerState).  Otherwise the static view (scale
        ``loss_scale``, every optimiser call counted as applied, the skipped count read from the device)."""
        if self.scaler is not None:
            return self.scaler.state()
        return {'scale': self.loss_scale, 'applied': self.optimizer.step_count, 'good_steps': 0, 'skipped': self.optimizer.skipped_steps()}

    def exchange_plan(self):
        """Per gradient-exchange group: its bytes and the point of the step at which its all-reduces are launched.  The LAST group is
        launched after the last backward kernel: its bytes are the exposed ones."""
        red = self.reducer
        plan = []
        for gid in sorted(set(red.bucket_group)):
            nbytes = 4 * sum(f.numel() for f, g in zip(red.flat, red.bucket_group) if g == gid)
            plan.append({'group': gid, 'bytes': nbytes, 'buckets': sum(1 for g in red.bucket_group if g == gid),
                         'launched_after_phase': PHASE_NAMES[gid]})
        total = sum(p['bytes'] for p in plan)
        return {'groups': plan, 'total_bytes': total, 'exposed_bytes': plan[-1]['bytes'], 'exposed_fraction': round(plan[-1]['bytes'] / total, 4)}

    # -- device work of one update ----------------------------------------------------------------------------------------
    def _forward_loss(self, inputs, targets, iteration, keep=None):
        """train.py:405-422 on a parsed micro-batch: RAW frame prosody for the consistency losses, conditioning, forward, loss."""
        raw_frames_energy, raw_frames_pitch = inputs[6], inputs[7]       # the frozen pitch predictor outputs RAW pitch
        if self.conditioner is not None:
            inputs = self.conditioner.process_batch(inputs, self.device)   # the length slots pass through untouched
        targets = (targets[0], inputs[3], inputs[4], targets[3], targets[4], targets[5], raw_frames_energy, raw_frames_pitch)
        outputs = self.model(inputs)
        result = self.criterion(outputs, targets, iteration)
        if keep is not None:                         # validate(keep_outputs=True): (targets, outputs) with tensors in the length slots
            outputs[2][3], outputs[3][1] = outputs[2][3].i64, outputs[3][1].i64
            keep.append((targets[:4] + (targets[4].i64,) + targets[5:], outputs))
        return result

    def _phases(self, parsed, iteration, launch):
        """zero the buckets; per micro-batch: forward, loss, backward phase A (everything downstream of the accent embedding).
        ``launch(gid)`` is called when group ``gid``'s gradients are complete.  Returns (loss summed over micro-batches, list of
        LossTerms, list of callables running the remaining phases B, C, D in order -- each ends with its own ``launch``)."""
        model, red, k = self.model, self.reducer, self.accumulation_steps
        rt = model.runtime
        red.zero_grad()
        ops.begin_step_arena(rt, self.device)       # one zero fill each for the step's small accumulators
        ops.begin_step_arena(self.criterion.runtime, self.device)
        rt.backward_split, rt.cut_levels = [], self.cut_levels
        tot, terms = None, []
        # d(what is differentiated) / d(loss) = loss scale / accumulation steps is folded into the loss kernels' own gradient outputs
        # (dynamic mode: the host part 1 / k, and the scale as the device scalar the loss launches multiply by)
        self.criterion.grad_scale = (1.0 / k, self.scaler.scale) if self.scaler is not None else self.loss_scale / k
        try:
            for inputs, targets in parsed:
                loss, indiv = self._forward_loss(inputs, targets, iteration)
                with red.accumulate(sync=False):                 # the exchange is launched explicitly, group by group
                    loss.backward(gradient=self._one)
                part = loss.detach() / k if k != 1 else loss.detach()
                tot = part if tot is None else tot + part
                terms.append(indiv)
        finally:
            cuts, rt.backward_split = rt.backward_split, None
            self.criterion.grad_scale = None
        ops.flush_wgrads(rt)                         # the FFT blocks' queued weight gradients, 8 layers per launch

        def end_arenas():
            ops.end_step_arena(rt)
            ops.end_step_arena(self.criterion.runtime)
        if self.cut_levels == 0:
            end_arenas()
        launch(0)

        def phase(level):
            def run():
                for lv, out, leaf in cuts:
                    if lv == level:
                        with red.accumulate(sync=False):
                            out.backward(leaf.grad)
                ops.flush_wgrads(rt)
                if level == self.cut_levels:
                    end_arenas()
                    cuts.clear()
                launch(level)
            return run
        return tot, terms, [phase(level) for level in range(1, self.cut_levels + 1)]

    def _parse(self, batches):
        parsed = [self._parse_one(b) for b in batches]
        key = (self.model.runtime.precision,) + tuple((tuple(i[0].shape), tuple(i[8].shape)) for i, _ in parsed)   # (B, L_max), (B, n_mel, T_max) per micro-batch
        return parsed, key

    def _parse_one(self, batch):
        """parse_batch -> (inputs, targets) with ONE ``Lengths`` per axis in the length slots (inputs[5], inputs[9] = targets[4]): model,
        loss and every backward Function of the micro-batch share it.  Bucketed mode: padded up to its bucket (pad_batch)."""
        inputs, _ = self.model.parse_batch(self.device, batch)
        if self.bucket is None:
            return _with_targets(inputs[:5] + (Lengths.of(inputs[5]),) + inputs[6:9] + (Lengths.of(inputs[9]),) + inputs[10:])
        L, T = inputs[0].shape[1], inputs[8].shape[2]
        return pad_batch(inputs, -(-L // self.bucket[0]) * self.bucket[0], -(-T // self.bucket[1]) * self.bucket[1])

    @staticmethod
    def _static_inputs(parsed):
        return [_with_targets(tuple(t.clone() for t in inputs)) for inputs, _ in parsed]      # (Lengths.clone: ``i32`` and ``exist`` too)

    def _capture(self, parsed, key):
        """One graph per backward phase for this padded shape.  One eager step on a side stream first (kernel attributes, weight
        packs, allocator), with the optimiser NOT applied: the captured step then sees the same state a replay will."""
        static = self._static_inputs(parsed)
        phase_a = lambda: self._phases(static, self.adv_weight, lambda gid: None)

        def whole_step():
            for run in phase_a()[2]:
                run()

        def first():
            self.model.runtime.seed_offset.add_(1)            # a new dropout stream per replay (the seeds in the launches are frozen)
            return phase_a()
        warm_up(whole_step)
        head, (loss, terms, rest) = capture(first)
        later = [capture(run, pool=head.pool())[0] for run in rest]      # phases B-D
        g = Entry([head] + later, inputs=static, loss=loss, terms_dev=[t._device_terms for t in terms])   # static device tensors: wrapped
        self.graphs[key] = g                                  # anew after every replay; a full cache drops its least used shape first
        return g

    def _check_conditioner(self):
        """A conditioner that had to RE-ALLOCATE its device tables (a speaker id beyond their rows) invalidates every captured graph:
        the graphs hold the old pointers and row count.  In-place refreshes (the normal case) need nothing."""
        gen = getattr(self.conditioner, 'generation', None)
        if gen != self._conditioner_generation:
            self.graphs.clear()
            self.val_graphs.clear()
            self._conditioner_generation = gen

    @staticmethod
    def _copy_static(si, inputs):
        """A micro-batch into the static input buffers of a graph (inputs of the same shapes; Lengths.copy_ for the length slots)."""
        for i, (dst, src) in enumerate(zip(si, inputs)):
            if i in (5, 9) or dst.data_ptr() != src.data_ptr():      # a batch built by resident_batch() already lives in the static buffers
                dst.copy_(src, non_blocking=True)

    def resident_batch(self, batch):
        """The batch copied into the static input buffers of its shape's graphs (captured now if need be) and handed back as a
        reference 14-tuple of THOSE tensors: ``train_step`` then finds its inputs in place (a data loader writing pinned host batches
        straight into the static buffers does the same).  One micro-batch per update only.  Not available in bucketed mode (ValueError):
        there the static buffers have the bucket's shape and the existence vectors, which a reference 14-tuple cannot carry."""
        if self.bucket is not None:
            raise ValueError('resident_batch() is not available in bucketed mode (Trainer(bucket=...)): pass the batch to train_step()')
        if self.accumulation_steps != 1 or not self.use_graphs:
            return batch
        self._check_conditioner()
        parsed, key = self._parse([batch])
        g = self.graphs.get(key) or self._capture(parsed, key)
        si = g.inputs[0][0]
        for dst, src in zip(si, parsed[0][0]):
            dst.copy_(src)
        out = list(si[:11]) + [batch[11], batch[12], si[11]]
        for i in (5, 9):                                      # a reference 14-tuple carries tensors: the host lengths go along as the hint
            out[i] = si[i].i64
            out[i]._dx_host_lengths = si[i].host
        return tuple(out)

    def train_step(self, batches):
        """``batches``: the ``accumulation_steps`` micro-batches (reference 14-tuples) of one parameter update.
        Returns (loss tensor = mean over micro-batches, list of per-micro-batch LossTerms, gradient norm tensor)."""
        batches = list(batches)
        if len(batches) != self.accumulation_steps:
            raise ValueError(f'expected {self.accumulation_steps} micro-batches, got {len(batches)}')
        parsed, key = self._parse(batches)
        red = self.reducer
        # a replayed graph reads the MFMA weight packs through frozen pointers and never runs the Python staleness check: anything that
        # changed the parameters since the last optimiser step (load_checkpoint, load_state_dict, an in-place edit) is re-packed here.
        # One launch when something is stale, nothing otherwise.
        ops.repack_all(self.model.runtime)
        if self.use_graphs:
            self._check_conditioner()
            self.adv_weight.fill_(self.criterion.update_adversarial_weight(self.iteration))
            g = self.graphs.get(key)
            if g is None:
                g = self._capture(parsed, key)
            g.hits += 1
            for (si, _), (inputs, _) in zip(g.inputs, parsed):
                self._copy_static(si, inputs)
            for gid, graph in enumerate(g.graphs):
                graph.replay()
                red.launch_group(gid)                         # exchanged (RCCL, its own stream) while the next phase's graph runs
            tot, terms = g.loss, [LossTerms(t) for t in g.terms_dev]
        else:
            tot, terms, rest = self._phases(parsed, self.iteration, red.launch_group)
            for run in rest:
                run()
        red.finish()
        if self.scaler is not None:                               # 1 / scale is read from the scaler state on the device
            grad_norm = self.optimizer.step(lr=self.learning_rate)
        else:
            grad_norm = self.optimizer.step(lr=self.learning_rate, grad_scale=1.0 / self.loss_scale)
        self.last_learning_rate = self.learning_rate
        self.iteration += 1
        self.learning_rate = update_learning_rate(self.hparams, self.iteration)
        return tot, terms, grad_norm

    # -- validation: train.py:163-209 ---------------------------------------------------------------------------------------
    def _val_forward(self, inputs, targets, keep=None):
        with torch.no_grad():
            return self._forward_loss(inputs, targets, self.val_adv_weight, keep)

    def validate(self, batches, keep_outputs=False):
        """The reference's ``validate`` (train.py:163-209, called at :474-491) on this rank's validation batches: eval mode (dropout
        off), no gradients, the same batch conditioning as training, ``iteration = 0`` in the loss (adversarial weight 0), losses
        averaged over the batches; every rank runs it, nothing is exchanged.  The device work of a batch is ONE captured graph per
        padded shape (forward + loss); the per-batch losses are summed on the device and fetched with one transfer at the end.
        Returns (val_loss, dict of the 7 averaged terms[, list of (targets, outputs) when ``keep_outputs``])."""
        model = self.model
        was_training = model.training
        model.eval()
        self._check_conditioner()
        ops.repack_all(model.runtime)
        tot = torch.zeros((), dtype=torch.float32, device=self.device)
        terms = torch.zeros(len(LossTerms.KEYS), dtype=torch.float32, device=self.device)
        kept, n = [], 0
        try:
            for batch in batches:
                inputs, targets = self._parse_one(batch)
                if keep_outputs or not self.use_graphs:      # the caller wants the tensors themselves: eager
                    loss, indiv = self._val_forward(inputs, targets, kept if keep_outputs else None)
                    tot += loss
                    terms += indiv._device_terms
                else:
                    key = (model.runtime.precision, tuple(inputs[0].shape), tuple(inputs[8].shape))
                    g = self.val_graphs.get(key)
                    if g is None:
                        g = self._capture_val([(inputs, targets)], key)
                    self._copy_static(g.inputs[0][0], inputs)
                    g.graphs[0].replay()
                    tot += g.loss
                    terms += g.terms_dev[0]
                n += 1
        finally:
            model.train(was_training)
        if n == 0:
            raise ValueError('validate() needs at least one batch')
        host = torch.cat([tot.reshape(1), terms]).div_(n).tolist()      # the one device -> host transfer of the validation pass
        out = (host[0], dict(zip(LossTerms.KEYS, host[1:])))
        return out + (kept,) if keep_outputs else out

    def _capture_val(self, parsed, key):
        static = self._static_inputs(parsed)
        forward = lambda: self._val_forward(*static[0])
        warm_up(forward)
        graph, (loss, indiv) = capture(forward)
        g = Entry([graph], inputs=static, loss=loss, terms_dev=[indiv._device_terms])
        self.val_graphs[key] = g                              # a full cache drops its oldest shape first
        return g

    def note_loss(self, value: float):
        """Host-side NaN bookkeeping for callers that fetch the loss (the reference skips logging, not the update)."""
        if math.isnan(value):
            self.nan_steps += 1

    # -- checkpoints: train.py:63-85 / :88-145 ---------------------------------------------------------------------------
    def checkpoint(self):
        cfg = {k: v for k, v in self.hparams.__dict__.items()}
        ck = {'iteration': self.iteration - 1, 'learning_rate': self.last_learning_rate, 'best_val_loss': self.best_val_loss,
              'state_dict': {k: v.detach().clone() for k, v in self.model.state_dict().items()},
              'optimizer': self.optimizer.state_dict(), 'config_params': cfg}
        if self.scaler is not None:                               # beside the reference's keys: four plain numbers
            ck['loss_scaler'] = dict(self.scaler.state().items())
        return ck

    def save_checkpoint(self, filepath):
        os.makedirs(os.path.dirname(os.path.abspath(filepath)), exist_ok=True)
        torch.save(self.checkpoint(), filepath)

    def load_checkpoint(self, checkpoint):
        """``checkpoint``: a path (read with ``weights_only=True``) or the dict itself.  Keys with DDP's ``module.`` prefix
        are accepted (train.py:272; consumers strip it, fine_tune.py:40)."""
        if isinstance(checkpoint, str):
            checkpoint = torch.load(checkpoint, map_location=self.device, weights_only=True)
        sd = {(k[7:] if k.startswith('module.') else k): v for k, v in checkpoint['state_dict'].items()}
        self.model.load_state_dict(sd)
        opt = checkpoint.get('optimizer')
        if opt is not None and len(opt['param_groups']) == len(self.optimizer.param_groups):
            self.optimizer.load_state_dict(opt)                          # else: keep the blank optimiser (train.py:127-133)
        if self.scaler is not None:
            # a checkpoint without the entry (an older one, the reference's own): the scale starts from hparams.loss_scale, the
            # bias-correction step from the optimiser state
            self.scaler.load(checkpoint.get('loss_scaler') or {'applied': self.optimizer.step_count})
        self.iteration = int(checkpoint['iteration']) + 1                # "next iteration is iteration + 1" (train.py:289)
        self.learning_rate = update_learning_rate(self.hparams, self.iteration)   # recomputed from the schedule (train.py:294)
        self.best_val_loss = checkpoint.get('best_val_loss', float('inf'))
        self.model.runtime.invalidate_packs()
