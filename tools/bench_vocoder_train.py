"""The HiFi-GAN generator's training step (forward with gradients + backward to every weight_g, weight_v, bias) at the reference's
training segment: B = 16 segments of 32 mel frames (8192 samples), synthetic weights, f32 operands.  One JSON line per configuration:

  * hip: forward and backward milliseconds (wall clock around a synchronised call), and one traced step's C-ABI launches split into
    conv (dx_voc_conv, dx_voc_post), wgrad (dx_voc_wgrad, dx_voc_post_bwd), elementwise (dx_voc_act_bwd) and pack (dx_voc_pack) with
    their counts and summed kernel times; 'glue_ms' is the rest of the traced step: torch's weight norm and padding, the flipped and
    three-tap weights built per step, allocation, autograd's own work;
  * torch: tests/vocoder_torch.py under torch autograd on the same GPU, same weights, same segment (fp32).

    python tools/bench_vocoder_train.py [v1] [v2] [v3] [--hip-only]          (no name: all three)
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tests import vocoder_helpers as vh  # noqa: E402
from tests import vocoder_torch  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import _lib, vocoder as voc  # noqa: E402

B, FRAMES = 16, 32
KINDS = {'dx_voc_conv': 'conv', 'dx_voc_post_c': 'conv', 'dx_voc_wgrad': 'wgrad', 'dx_voc_post_bwd': 'wgrad', 'dx_voc_act_bwd': 'elementwise',
         'dx_voc_pack': 'pack'}


def timed(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def split(records):
    out = {}
    for name, _, a, b in records:
        kind = KINDS.get(name, name)
        row = out.setdefault(kind, {'launches': 0, 'ms': 0.0})
        row['launches'] += 1
        row['ms'] += a.elapsed_time(b)
    return {k: {'launches': v['launches'], 'ms': round(v['ms'], 3)} for k, v in out.items()}


def traced(fn):
    """-> (C-ABI launches by kind, wall ms) of one synchronised call of fn with every launch bracketed by events"""
    recs = []
    torch.cuda.synchronize()
    old = _lib.set_timer(recs)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    _lib.set_timer(old)
    return out, split(recs), wall


def bench(name, hip_only):
    dev = 'cuda'
    cfg = voc.CONFIGS[name]()
    g = torch.Generator().manual_seed(3)
    mel = ((torch.randn(B, 80, FRAMES, generator=g) * 1.5 - 5.0).clamp(-11.5, 2.0)).to(dev)
    dy = torch.randn(B, 1, FRAMES * voc.HOP, generator=g).to(dev)
    gen = voc.HiFiGANGenerator(cfg).to(dev)
    gen.load_state_dict(vh.state_dict(name))
    out = {'config': name, 'workload': f'B={B} segments of {FRAMES} frames ({FRAMES * voc.HOP} samples), f32'}

    def step():
        gen.zero_grad(set_to_none=True)
        gen(mel).backward(dy)

    def forward_only():
        return gen(mel)

    fwd = timed(forward_only)
    both = timed(step)
    y, fwd_split, fwd_wall = traced(forward_only)
    gen.zero_grad(set_to_none=True)
    _, bwd_split, bwd_wall = traced(lambda: y.backward(dy))
    kernels = lambda s: sum(v['ms'] for v in s.values())
    out['hip'] = {'forward_ms': round(fwd, 3), 'backward_ms': round(both - fwd, 3), 'step_ms': round(both, 3),
                  'forward_launches': fwd_split, 'backward_launches': bwd_split,
                  'forward_glue_ms': round(fwd_wall - kernels(fwd_split), 3), 'backward_glue_ms': round(bwd_wall - kernels(bwd_split), 3),
                  'peak_memory_mb': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    if not hip_only:
        params = {k: v.detach().clone().requires_grad_(True) for k, v in gen.state_dict().items()}
        names = gen.layer_names()

        def torch_forward():
            weights = {n: (torch._weight_norm(params[n + '.weight_v'], params[n + '.weight_g'], 0), params[n + '.bias']) for n in names}
            return vocoder_torch.generator(mel, weights, cfg)

        def torch_step():
            for p in params.values():
                p.grad = None
            torch_forward().backward(dy[:, 0])

        tf = timed(torch_forward)
        ts = timed(torch_step)
        out['torch'] = {'forward_ms': round(tf, 3), 'backward_ms': round(ts - tf, 3), 'step_ms': round(ts, 3)}
        out['hip_over_torch_step'] = round(ts / both, 2)
    print(json.dumps(out), flush=True)


def main():
    names = [a for a in sys.argv[1:] if a in voc.CONFIGS] or ['v1', 'v2', 'v3']
    for name in names:
        bench(name, '--hip-only' in sys.argv)


if __name__ == '__main__':
    main()
