"""The float64 yardstick of the fused weight-norm AdamW step (csrc/dx_vocoder_optim.hip), its torch counterpart, the test inputs and
the bar.  CPU only; shared by test_finetune_cpu.py, test_vocoder_optim_gpu.py and test_finetune_gpu.py."""
import math

import torch

REFERENCE_HYPER = (2e-4, (0.8, 0.99), 1e-8, 0.01)            # torch.optim.AdamW as finetune_hifigan.py:130-135 configures it
EXAGGERATED_HYPER = (2.0 ** -4, (0.5, 0.75), 1e-3, 0.25)     # every term of the update (decay, bias corrections, eps) >= 1e-3 of the parameter
HYPERS = {'reference': REFERENCE_HYPER, 'exaggerated': EXAGGERATED_HYPER}
NORMED_SHAPES = ((32, 5), (128, 15), (7, 123), (64, 328), (1, 224), (1, 3072), (33, 1300), (16, 5120))
PLAIN_SIZES = (1, 32, 1027)
NORMED_KEYS = ('m_v', 's_v', 'm_g', 's_g', 'W', 'v', 'g')
PLAIN_KEYS = ('m', 's', 'p')
EPS32 = 2.0 ** -24


def adamw_reference(p, grad, m, s, step, hyper, dtype=torch.float64):
    """torch.optim.AdamW's definition on one tensor -> (p', m', s')."""
    lr, (b1, b2), eps, wd = hyper
    p, grad, m, s = (t.to(dtype) for t in (p, grad, m, s))
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * grad
    s = b2 * s + (1 - b2) * grad * grad
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p = p - (lr / bc1) * (m / (s.sqrt() / math.sqrt(bc2) + eps))
    return p, m, s


def wn_gradients(v, g, dW, dtype=torch.float64):
    """The weight norm's backward: v (R, ...), g (R, 1, ...), dW in v's layout -> (dv like v, dg like g)."""
    R = v.shape[0]
    v2, g2, d2 = v.to(dtype).reshape(R, -1), g.to(dtype).reshape(R, 1), dW.to(dtype).reshape(R, -1)
    nrm = (v2 * v2).sum(1, keepdim=True).sqrt()
    dg = (d2 * v2).sum(1, keepdim=True) / nrm
    dv = (g2 / nrm) * (d2 - (dg / nrm) * v2)
    return dv.reshape(v.shape), dg.reshape(g.shape)


def wn_adamw_reference(v, g, dW, moments, step, hyper, dtype=torch.float64):
    """The formulas of include/daft_exprt_hip.h (dx_wn_adamw) in torch.  moments: (m_v, s_v, m_g, s_g) -> {v, g, m_v, s_v, m_g, s_g, W}."""
    m_v, s_v, m_g, s_g = moments
    dv, dg = wn_gradients(v, g, dW, dtype)
    g1, m_g1, s_g1 = adamw_reference(g, dg, m_g, s_g, step, hyper, dtype)
    v1, m_v1, s_v1 = adamw_reference(v, dv, m_v, s_v, step, hyper, dtype)
    R = v.shape[0]
    nrm = (v1.reshape(R, -1) ** 2).sum(1).sqrt().reshape(g1.shape)
    return dict(v=v1, g=g1, m_v=m_v1, s_v=s_v1, m_g=m_g1, s_g=s_g1, W=v1 * (g1 / nrm))


def _torch_optimizer(params, states, step, hyper):
    lr, betas, eps, wd = hyper
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    sd = opt.state_dict()
    sd['state'] = {i: {'step': torch.tensor(float(step - 1)), 'exp_avg': m.clone(), 'exp_avg_sq': s.clone()} for i, (m, s) in enumerate(states)}
    opt.load_state_dict(sd)
    return opt


def torch_wn_adamw(v, g, dW, moments, step, hyper, dtype, steps=1):
    """torch's own: ``torch._weight_norm`` under autograd and ``torch.optim.AdamW`` with a loaded state, ``steps`` steps on the same
    dW -> the same dict as wn_adamw_reference."""
    m_v, s_v, m_g, s_g = (t.to(dtype) for t in moments)
    vp, gp = torch.nn.Parameter(v.to(dtype).clone()), torch.nn.Parameter(g.to(dtype).clone())
    opt = _torch_optimizer([gp, vp], [(m_g, s_g), (m_v, s_v)], step, hyper)
    for _ in range(steps):
        opt.zero_grad()
        torch._weight_norm(vp, gp, 0).backward(dW.to(dtype))
        opt.step()
    st = opt.state_dict()['state']
    return dict(v=vp.detach(), g=gp.detach(), m_v=st[1]['exp_avg'], s_v=st[1]['exp_avg_sq'], m_g=st[0]['exp_avg'], s_g=st[0]['exp_avg_sq'],
                W=torch._weight_norm(vp, gp, 0).detach())


def torch_adamw(p, grad, m, s, step, hyper, dtype, steps=1):
    pp = torch.nn.Parameter(p.to(dtype).clone())
    opt = _torch_optimizer([pp], [(m.to(dtype), s.to(dtype))], step, hyper)
    for _ in range(steps):
        pp.grad = grad.to(dtype).clone()
        opt.step()
    st = opt.state_dict()['state'][0]
    return dict(p=pp.detach(), m=st['exp_avg'], s=st['exp_avg_sq'])


def plain_reference(p, grad, m, s, step, hyper, dtype=torch.float64):
    p1, m1, s1 = adamw_reference(p, grad, m, s, step, hyper, dtype)
    return dict(p=p1, m=m1, s=s1)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _warm(grad64, gen):
    """Warm moments for a tensor whose float64 gradient is grad64: exp_avg_sq in [1, 4] x the gradient's mean square, so that the update
    is Lipschitz in the gradient and no element needs excluding."""
    ms = float((grad64 * grad64).mean())
    s = (1 + 3 * torch.rand(grad64.shape, generator=gen, dtype=torch.float64)) * ms
    m = 0.5 * math.sqrt(ms) * torch.randn(grad64.shape, generator=gen, dtype=torch.float64)
    return m.float(), s.float()


def normed_inputs(R, n, seed, warm=True):
    """fp32 CPU inputs of one weight-normed job: dict v (R, n), g (R, 1), dW (R, n), m_v, s_v, m_g, s_g; |v| and g below 1."""
    gen = torch.Generator().manual_seed(seed)
    v = (torch.rand(R, n, generator=gen) - 0.5).float()
    g = (0.5 + 0.45 * torch.rand(R, 1, generator=gen)).float()
    dW = torch.randn(R, n, generator=gen).float()
    dv, dg = wn_gradients(v, g, dW)
    if warm:
        m_v, s_v = _warm(dv, gen)
        m_g, s_g = _warm(dg, gen)
    else:
        m_v, s_v, m_g, s_g = torch.zeros(R, n), torch.zeros(R, n), torch.zeros(R, 1), torch.zeros(R, 1)
    return dict(v=v, g=g, dW=dW, m_v=m_v, s_v=s_v, m_g=m_g, s_g=s_g)


def plain_inputs(n, seed, warm=True):
    gen = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, generator=gen) - 0.5).float()
    grad = torch.randn(n, generator=gen).float()
    m, s = _warm(grad.double(), gen) if warm else (torch.zeros(n), torch.zeros(n))
    return dict(p=p, dW=grad, m=m, s=s)


def all_inputs(seed=0, warm=True):
    """The eleven jobs of the table test, in order: the eight weight-normed shapes, then the three plain sizes."""
    jobs = [normed_inputs(R, n, seed + 17 * i, warm) for i, (R, n) in enumerate(NORMED_SHAPES)]
    return jobs + [plain_inputs(n, seed + 1000 + i, warm) for i, n in enumerate(PLAIN_SIZES)]


def references(job, step, hyper):
    """-> (float64 result, torch's own float32 CPU result) of one job's inputs."""
    if 'v' in job:
        mo = (job['m_v'], job['s_v'], job['m_g'], job['s_g'])
        return wn_adamw_reference(job['v'], job['g'], job['dW'], mo, step, hyper), torch_wn_adamw(job['v'], job['g'], job['dW'], mo, step, hyper, torch.float32)
    return plain_reference(job['p'], job['dW'], job['m'], job['s'], step, hyper), torch_adamw(job['p'], job['dW'], job['m'], job['s'], step, hyper, torch.float32)


# ---- the bar ----------------------------------------------------------------------------------------------------------------------
def bar_ratio(key, got, ref64, ref32, before=None):
    """max|d| / (4 max|spread| + 4 * 2^-24 * max|scale|): d = got - float64, spread = torch's float32 run - float64.  For a parameter
    (``before`` given: its fp32 value ahead of the step) d and spread are those of the UPDATE p' - p, taken in float64 from the stored
    values, and the scale is the parameter; otherwise the scale is the float64 result."""
    got, ref64, ref32 = got.double().reshape(-1), ref64.double().reshape(-1), ref32.double().reshape(-1)
    if before is not None:
        p = before.double().reshape(-1)
        d, spread, scale = (got - p) - (ref64 - p), (ref32 - p) - (ref64 - p), p
    else:
        d, spread, scale = got - ref64, ref32 - ref64, ref64
    assert torch.isfinite(got).all(), key
    bound = 4 * float(spread.abs().max()) + 4 * EPS32 * float(scale.abs().max())
    return float(d.abs().max()) / bound


def job_ratios(job, got, ref64, ref32):
    """-> {quantity: bar ratio} for every output tensor class of one job."""
    out = {}
    for key in (NORMED_KEYS if 'v' in job else PLAIN_KEYS):
        before = job[key] if key in ('v', 'g', 'p') else None
        out[key] = bar_ratio(key, got[key], ref64[key], ref32[key], before)
    return out
