"""HiFi-GAN discriminators at the fine-tuning shape: B = 16 segments of 8192 samples, real and generated, synthetic weights.
One JSON line: the time of ``HiFiGanDiscriminators.losses`` (both discriminators on both inputs + the six losses; f32 and bf16), of the
plain-torch restatement tests/disc_torch.py on the same GPU (fp32, and bf16 tensors), the FLOPs of one pass recomputed by
profiling.price() from the launches themselves, and per-kernel times with TFLOP/s (MFMA kernels) or GB/s (the others).

Times are host clocks around work that ends in a device synchronise, after warm-up; the per-kernel figures bracket each launch with
events (profiling.py), in a pass of their own.  Needs a GPU: there is no fallback.

    python tools/bench_discriminators.py [--backward | --train]

``--backward`` measures the generator side instead: ``losses()``, ``generator_loss_grad()`` (the same pass + the backward to the
generated waveform), the per-kernel split of the backward, and torch autograd of the restatement (forward + backward) on the same GPU.

``--train`` measures the discriminator step (f32): ``losses()``, ``discriminator_loss_grad(power_iterations=0)`` (the same pass + the
gradient of loss_disc to all 154 parameters), the per-kernel split of the step, and torch fp32 autograd of the restatement from the
folded weights to loss_disc (forward + backward to the 56 folded (weight, bias) pairs) on the same GPU.
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tests import disc_helpers as dh  # noqa: E402
from tests import disc_torch  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import _lib, discriminators as disc, profiling  # noqa: E402

B, T = 16, 8192


def timed(fn, n=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def backward_main():
    from tests import disc_backward_torch as dbt
    dev = 'cuda'
    y, y_hat = (t.to(dev) for t in dh.make_inputs(T, 9, batch=B))
    states = dh.state_dicts()
    out = {'workload': f'B={B} segments of {T} samples, real + generated; gradient to the generated half'}
    geom = profiling.Geometry([[1]])
    for prec in ('f32', 'bf16'):
        D = disc.HiFiGanDiscriminators(states, device=dev, precision=prec)
        with torch.no_grad():
            t_fwd = timed(lambda: D.losses(y, y_hat))
        t_all = timed(lambda: D.generator_loss_grad(y, y_hat))
        recs = []
        old = _lib.set_timer(recs)
        D.generator_loss_grad(y, y_hat)
        _lib.set_timer(old)
        torch.cuda.synchronize()
        bwd = [r for r in recs if r[0] in ('dx_disc_conv_dgrad', 'dx_disc_post_bwd', 'dx_disc_first_bwd', 'dx_disc_pool_bwd')]
        flops = sum(profiling.price(name, args, geom)[2] or 0.0 for name, args, _, _ in bwd)
        out[f'hip_{prec}'] = {'losses_s': round(t_fwd, 6), 'generator_loss_grad_s': round(t_all, 6), 'backward_s': round(t_all - t_fwd, 6),
                              'backward_launches': len(bwd), 'backward_tflop': round(flops / 1e12, 4)}
        out[f'profile_backward_{prec}'] = profiling.summarize(bwd, geom, prec)
        out[f'profile_forward_{prec}'] = profiling.summarize([r for r in recs if r not in bwd], geom, prec)
    mpd_w = {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]).to(dev), b.to(dev)) for k, (w, b) in disc.fold_state_dict(states['mpd']).items()}
    msd_w = {k: (w.to(dev), b.to(dev)) for k, (w, b) in disc.fold_state_dict(states['msd']).items()}
    out['torch_fp32_autograd'] = {'s': round(timed(lambda: dbt.autograd_grad(y, y_hat, mpd_w, msd_w, (1, 1, 1, 1), torch.float32), n=5, warm=2), 6)}
    out['hip_f32_over_torch_fp32'] = round(out['torch_fp32_autograd']['s'] / out['hip_f32']['generator_loss_grad_s'], 2)
    print(json.dumps(out))


STEP_KERNELS = ('dx_disc_wgrad', 'dx_disc_post_wgrad', 'dx_disc_first_wgrad', 'dx_disc_conv_dgrad', 'dx_disc_dgrad_pack')


def train_main():
    dev = 'cuda'
    y, y_hat = (t.to(dev) for t in dh.make_inputs(T, 9, batch=B))
    states = dh.state_dicts()
    out = {'workload': f'B={B} segments of {T} samples, real + generated; loss_disc to all 154 parameters'}
    geom = profiling.Geometry([[1]])
    D = disc.HiFiGanDiscriminators(states, device=dev)
    with torch.no_grad():
        t_fwd = timed(lambda: D.losses(y, y_hat))
    t_all = timed(lambda: D.discriminator_loss_grad(y, y_hat, power_iterations=0))
    recs = []
    old = _lib.set_timer(recs)
    D.discriminator_loss_grad(y, y_hat, power_iterations=0)
    _lib.set_timer(old)
    torch.cuda.synchronize()
    step = [r for r in recs if r[0] in STEP_KERNELS]
    flops = sum(profiling.price(name, args, geom)[2] or 0.0 for name, args, _, _ in step)
    out['hip_f32'] = {'losses_s': round(t_fwd, 6), 'discriminator_loss_grad_s': round(t_all, 6), 'step_s': round(t_all - t_fwd, 6),
                      'step_launches': len(step), 'step_tflop': round(flops / 1e12, 4), 'over_losses': round(t_all / t_fwd, 2)}
    out['profile_step_f32'] = profiling.summarize(step, geom, 'f32')
    layers = {}                                     # the weight-gradient launches by layer class: [launches, us, FLOPs]
    for name, args, ev0, ev1 in step:
        if name == 'dx_disc_wgrad':
            key = '{Cin}->{Cout} k{taps} s{stride} g{groups}'.format(**args)
            e = layers.setdefault(key, [0, 0.0, 0.0])
            e[0] += 1
            e[1] += ev0.elapsed_time(ev1) * 1e3
            e[2] += profiling.price(name, args, geom)[2]
    out['wgrad_by_layer_class'] = {k: {'launches': n, 'total_us': round(us, 1), 'tflops': round(fl / us / 1e6, 2)} for k, (n, us, fl) in layers.items()}
    folded ={'mpd': {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]).to(dev), b.to(dev)) for k, (w, b) in disc.fold_state_dict(states['mpd']).items()},
              'msd': {k: (w.to(dev), b.to(dev)) for k, (w, b) in disc.fold_state_dict(states['msd']).items()}}

    def autograd():
        leaves = {d: {k: (w.detach().requires_grad_(True), b.detach().requires_grad_(True)) for k, (w, b) in f.items()} for d, f in folded.items()}
        six = disc_torch.six_losses(disc_torch.mpd(y, y_hat, leaves['mpd']), disc_torch.msd(y, y_hat, leaves['msd']))
        (six['loss_disc_f'] + six['loss_disc_s']).backward()
        return leaves
    out['torch_fp32_autograd'] = {'s': round(timed(autograd, n=5, warm=2), 6)}
    out['hip_f32_over_torch_fp32'] = round(out['torch_fp32_autograd']['s'] / out['hip_f32']['discriminator_loss_grad_s'], 2)
    print(json.dumps(out))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_discriminators needs a GPU')
    if '--backward' in sys.argv[1:]:
        return backward_main()
    if '--train' in sys.argv[1:]:
        return train_main()
    dev = 'cuda'
    y, y_hat = (t.to(dev) for t in dh.make_inputs(T, 9, batch=B))
    states = dh.state_dicts()
    out = {'workload': f'B={B} segments of {T} samples, real + generated'}
    geom = profiling.Geometry([[1]])
    with torch.no_grad():
        for prec in ('f32', 'bf16'):
            D = disc.HiFiGanDiscriminators(states, device=dev, precision=prec)
            t = timed(lambda: D.losses(y, y_hat))
            recs = []
            old = _lib.set_timer(recs)
            D.losses(y, y_hat)
            _lib.set_timer(old)
            torch.cuda.synchronize()
            flops = sum(profiling.price(name, args, geom)[2] or 0.0 for name, args, _, _ in recs)
            out[f'hip_{prec}'] = {'s': round(t, 6), 'launches': len(recs), 'tflop_per_pass': round(flops / 1e12, 4),
                                  'tflops': round(flops / t / 1e12, 2)}
            out[f'profile_{prec}'] = profiling.summarize(recs, geom, prec)
        folded = {'mpd': {k: (w.reshape(w.shape[0], w.shape[1], w.shape[2]).to(dev), b.to(dev)) for k, (w, b) in disc.fold_state_dict(states['mpd']).items()},
                  'msd': {k: (w.to(dev), b.to(dev)) for k, (w, b) in disc.fold_state_dict(states['msd']).items()}}
        for tag, dtype in (('torch_fp32', torch.float32), ('torch_bf16', torch.bfloat16)):
            yy, yh = y.to(dtype), y_hat.to(dtype)

            def run():
                return disc_torch.six_losses(disc_torch.mpd(yy, yh, folded['mpd'], dtype), disc_torch.msd(yy, yh, folded['msd'], dtype))
            out[tag] = {'s': round(timed(run, n=5, warm=2), 6)}
        out['hip_f32_over_torch_fp32'] = round(out['torch_fp32']['s'] / out['hip_f32']['s'], 2)
        out['hip_bf16_over_torch_bf16'] = round(out['torch_bf16']['s'] / out['hip_bf16']['s'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
