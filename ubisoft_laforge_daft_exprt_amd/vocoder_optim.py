"""AdamW for the HiFi-GAN models: the weight norm's backward, the step and the re-fold of every layer in ONE launch.

Reference behaviour: ``torch.optim.AdamW(generator.parameters(), lr, betas=(adam_b1, adam_b2))`` and the same over
``itertools.chain(msd.parameters(), mpd.parameters())`` (vocoder/finetune_hifigan.py:130-135), stepped at :226 and :243, with
``torch.nn.utils.weight_norm`` folding every layer under autograd.  Here a weight-normed layer hands over the gradient of its FOLDED
weight; ``dx_wn_adamw`` (csrc/dx_vocoder_optim.hip) derives the gradients of ``weight_g`` and ``weight_v`` from it, steps both and
writes the new folded weight into ``W``, a buffer this object owns and the convolution packs are built from.  Biases and the
spectral-normed ``weight_orig`` are plain AdamW jobs of the same launch.

``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.AdamW``'s layout, indexed by the modules' ``parameters()`` in order (a
weight-normed layer: bias, weight_g, weight_v), so the ``optim_g`` / ``optim_d`` entries of a reference ``do_*`` checkpoint load here
and what is saved here loads into torch.
"""
from __future__ import annotations

import torch

from ._lib import lib, stream as _stream

# {address of a device job table: (elements of its weight-normed jobs, elements of its plain jobs)}: what profiling.price needs
TABLE_LOG = {}


def _check_param(name, p):
    if p.dtype != torch.float32 or p.device.type != 'cuda' or not p.is_contiguous():
        raise ValueError(f'NormedAdamW: {name} must be a contiguous fp32 tensor on the GPU, got {p.dtype} on {p.device}')


class NormedAdamW:
    """``named_layers``: (name, module) pairs in the order the reference hands their parameters to AdamW; a module owns ``bias`` and
    either ``weight_g`` / ``weight_v`` (weight norm over everything but dim 0) or ``weight_orig`` (spectral norm: its ``W / sigma`` stays
    with the caller).  The parameters must already be on the GPU; they are written in place, through raw pointers, and never move.

    ``step(grads)``: ``{name: (dW, db)}`` for a weight-normed layer -- dW the gradient of the folded weight in ``weight_v``'s memory
    layout --, ``{name + '.bias': g, name + '.weight_orig': g}`` for a spectral-normed one.  One launch, no host synchronisation.  The
    job table lives in device memory; its gradient column is uploaded again (a pinned, asynchronous copy of under 0.2 MB) only when a
    gradient arrives at another address than last time.
    ``fold()``: ``W`` of every weight-normed layer from the stored g and v (``dx_wn_fold``: the step's own fold, the same bits).
    ``folded()`` -> ``{name: (W, bias)}`` for the weight-normed layers: views of this object's buffers, not copies.
    ``leaves=True`` makes every ``W`` a ``requires_grad`` leaf: the generator's forward takes them, ``backward()`` leaves dW in ``.grad``.
    ``lr`` is a plain float the caller may set.  Whoever steps must drop what was derived from the old weights (convolution packs, the
    generator's no-grad cache): a raw write bumps no version counter."""

    def __init__(self, named_layers, lr, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01, leaves=False):
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.initial_lr = float(lr)
        self.step_count = 0
        self.params, self.keys = [], []              # torch's order: every nn.Parameter, and the key its gradient arrives under
        self.normed, self.plain = [], []             # (name, g, v, index of g in params) / (key, p, index in params)
        for name, module in named_layers:
            own = dict(module.named_parameters(recurse=False))
            if set(own) == {'bias', 'weight_g', 'weight_v'}:
                if list(own) != ['bias', 'weight_g', 'weight_v']:
                    raise ValueError(f'NormedAdamW: {name}: parameters in the order bias, weight_g, weight_v expected, got {list(own)}')
                for k, p in own.items():             # registration order: bias, weight_g, weight_v
                    _check_param(f'{name}.{k}', p)
                    if k == 'bias':
                        self.plain.append((name + '.bias', p, len(self.params)))
                    elif k == 'weight_g':
                        if p.numel() != own['weight_v'].shape[0]:
                            raise ValueError(f'NormedAdamW: {name}: weight_g must hold one norm per row of weight_v (dim 0)')
                        self.normed.append((name, p, own['weight_v'], len(self.params)))
                    self.params.append(p)
                    self.keys.append(f'{name}.{k}')
            elif set(own) == {'bias', 'weight_orig'}:
                for k, p in own.items():
                    _check_param(f'{name}.{k}', p)
                    self.plain.append((f'{name}.{k}', p, len(self.params)))
                    self.params.append(p)
                    self.keys.append(f'{name}.{k}')
            else:
                raise ValueError(f'NormedAdamW: {name}: a layer owns bias and weight_g / weight_v, or bias and weight_orig; got {sorted(own)}')
        if not self.params:
            raise ValueError('NormedAdamW: no layers')
        self.device = self.params[0].device
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.W = {name: torch.empty_like(v).requires_grad_(bool(leaves)) for name, _, v, _ in self.normed}
        self._jobs = self._job_rows()
        self._grad_key = None
        self._table = None
        self._upload([r[5] for r in self._jobs])     # placeholders in the gradient column until the first step: fold() reads none
        self.fold()

    # -- the job table -------------------------------------------------------------------------------------------------------------
    def _job_rows(self):
        """One row of 11 integers per job (include/daft_exprt_hip.h), the gradient column holding the parameter's own address."""
        rows = []
        for name, g, v, i in self.normed:
            R = v.shape[0]
            rows.append([1, R, v.numel() // R, v.data_ptr(), g.data_ptr(), v.data_ptr(), self.exp_avg[i + 1].data_ptr(),
                         self.exp_avg_sq[i + 1].data_ptr(), self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(), self.W[name].data_ptr()])
        for key, p, i in self.plain:
            rows.append([0, 1, p.numel(), p.data_ptr(), 0, p.data_ptr(), self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(), 0, 0, 0])
        return rows

    def _upload(self, grad_ptrs):
        L = lib()
        for row, ptr in zip(self._jobs, grad_ptrs):
            row[5] = ptr
        jobs = torch.tensor(self._jobs, dtype=torch.int64)
        nbytes, blocks = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
        L.dx_wn_adamw_table_size(jobs.data_ptr(), len(self._jobs), nbytes.data_ptr(), blocks.data_ptr())
        host = torch.empty(int(nbytes.item()), dtype=torch.uint8).pin_memory()
        L.dx_wn_adamw_table(jobs.data_ptr(), len(self._jobs), host.data_ptr(), host.numel())
        if self._table is None:
            self._table = torch.empty(host.numel(), dtype=torch.uint8, device=self.device)
            TABLE_LOG[self._table.data_ptr()] = (sum(v.numel() for _, _, v, _ in self.normed), sum(p.numel() for _, p, _ in self.plain))
        self._table.copy_(host, non_blocking=True)   # the pinned block is not reused before this copy has run
        self._blocks = int(blocks.item())

    def __del__(self):
        if getattr(self, '_table', None) is not None:
            TABLE_LOG.pop(self._table.data_ptr(), None)

    # -- the launches --------------------------------------------------------------------------------------------------------------
    def _gradients(self, grads):
        out = []
        for name, g, v, _ in self.normed:
            dW = grads[name][0]
            if dW.numel() != v.numel() or dW.dtype != torch.float32 or dW.device != v.device:
                raise ValueError(f'NormedAdamW.step: the gradient of {name} must be fp32 with weight_v\'s {v.numel()} elements on {v.device}, '
                                 f'got {tuple(dW.shape)} {dW.dtype} on {dW.device}')
            out.append(dW if dW.is_contiguous() else dW.contiguous())
        for key, p, _ in self.plain:
            layer = key[:-len('.bias')] if key.endswith('.bias') else None
            d = grads[layer][1] if layer is not None and layer in grads and isinstance(grads[layer], (tuple, list)) else grads[key]
            if d.numel() != p.numel() or d.dtype != torch.float32 or d.device != p.device:
                raise ValueError(f'NormedAdamW.step: the gradient of {key} must be fp32 with {p.numel()} elements on {p.device}, '
                                 f'got {tuple(d.shape)} {d.dtype} on {d.device}')
            out.append(d if d.is_contiguous() else d.contiguous())
        return out

    def step(self, grads):
        with torch.no_grad():
            g = self._gradients(grads)                   # kept alive until the launch is issued; the allocator orders reuse on this stream
            key = tuple(t.data_ptr() for t in g)
            if key != self._grad_key:
                self._upload(key)
                self._grad_key = key
            self.step_count += 1
            lib().dx_wn_adamw(self._table.data_ptr(), len(self._jobs), self._blocks, self.lr, self.betas[0], self.betas[1], self.eps,
                              self.weight_decay, self.step_count, _stream(self.device))

    def fold(self):
        lib().dx_wn_fold(self._table.data_ptr(), len(self._jobs), self._blocks, _stream(self.device))

    def folded(self) -> dict:
        bias = {key[:-len('.bias')]: p for key, p, _ in self.plain if key.endswith('.bias')}
        return {name: (self.W[name], bias[name]) for name, _, _, _ in self.normed}

    def zero_grad(self):
        """Drops ``.grad`` of the folded leaves and of the parameters (``leaves=True``: autograd would otherwise add into them)."""
        for w in self.W.values():
            w.grad = None
        for p in self.params:
            p.grad = None

    # -- checkpoint layout of torch.optim.AdamW ------------------------------------------------------------------------------------
    @property
    def param_groups(self):
        return [{'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay, 'amsgrad': False,
                 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                 'decoupled_weight_decay': True, 'initial_lr': self.initial_lr, 'params': list(range(len(self.params)))}]

    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i in range(len(self.params)):
                state[i] = {'step': torch.tensor(float(self.step_count)), 'exp_avg': self.exp_avg[i].clone(),
                            'exp_avg_sq': self.exp_avg_sq[i].clone()}
        return {'state': state, 'param_groups': self.param_groups}

    def load_state_dict(self, sd):
        """Raises ValueError when the state does not fit these parameters (count, shapes, one common step); nothing is changed then."""
        groups = sd.get('param_groups') if isinstance(sd, dict) else None
        if not groups or 'state' not in sd:
            raise ValueError("NormedAdamW: an optimizer state is {'state': ..., 'param_groups': [...]}")
        if len(groups) != 1 or len(groups[0]['params']) != len(self.params):
            raise ValueError(f'NormedAdamW: the optimizer state has {sum(len(g["params"]) for g in groups)} parameters in {len(groups)} groups; '
                             f'these modules have {len(self.params)} in one group')
        g = groups[0]
        if g.get('amsgrad') or g.get('maximize'):
            raise ValueError('NormedAdamW: amsgrad and maximize are not built')
        steps, loaded = set(), []
        for idx, i in enumerate(g['params']):
            st = sd['state'].get(i)
            if st is None:
                loaded.append(None)
                continue
            p = self.params[idx]
            if tuple(st['exp_avg'].shape) != tuple(p.shape) or tuple(st['exp_avg_sq'].shape) != tuple(p.shape):
                raise ValueError(f'NormedAdamW: state {i} has moments of shape {tuple(st["exp_avg"].shape)}; {self.keys[idx]} is {tuple(p.shape)}')
            steps.add(int(st['step']))
            loaded.append(st)
        if len(steps) > 1 or (steps and any(st is None for st in loaded)):
            raise ValueError(f'NormedAdamW: per-parameter step counts differ ({sorted(steps)}, or some parameters have no state): the fused '
                             f'kernel keeps ONE bias-correction step')
        with torch.no_grad():
            for idx, st in enumerate(loaded):
                if st is None:
                    self.exp_avg[idx].zero_()
                    self.exp_avg_sq[idx].zero_()
                else:
                    self.exp_avg[idx].copy_(st['exp_avg'])
                    self.exp_avg_sq[idx].copy_(st['exp_avg_sq'])
        self.step_count = steps.pop() if steps else 0
        self.lr = float(g.get('lr', self.lr))
        self.initial_lr = float(g.get('initial_lr', self.lr))
        self.betas = tuple(float(b) for b in g.get('betas', self.betas))
        self.eps, self.weight_decay = float(g.get('eps', self.eps)), float(g.get('weight_decay', self.weight_decay))


__all__ = ['NormedAdamW']
