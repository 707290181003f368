"""bench.py's contract with the tools that read it: ``--steps`` timed steps, ``ms_per_step`` in the one JSON line, and
``--dump-outputs DIR`` writing what the last timed step returned as float32 .npy files (< 64 MB, the same positions every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP_NAMES = ('loss', 'loss_terms', 'grad_norm', 'params_sample', 'grads_sample')
DUMP_LIMIT = 64 << 20


def _dump_sizes(out_dir):
    files = sorted(os.listdir(out_dir))
    assert files == sorted(n + '.npy' for n in DUMP_NAMES)
    arrays = {n: np.load(os.path.join(out_dir, n + '.npy')) for n in DUMP_NAMES}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) < DUMP_LIMIT
    return arrays


def test_dump_outputs_is_a_fixed_sample_of_what_the_step_returned(tmp_path):
    """On CPU tensors (no compute call): the files, their dtype and size, and the sampled positions are the same positions of the
    parameters and gradients, flattened in named_parameters() order, on every call."""
    import bench
    import ubisoft_laforge_daft_exprt_amd as pkg
    from ubisoft_laforge_daft_exprt_amd.loss import LossTerms
    from ubisoft_laforge_daft_exprt_amd.synth import synthetic_state_dict
    model = pkg.DaftExprt(pkg.HyperParams(n_speakers=2))
    model.load_state_dict(synthetic_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1234), strict=True)
    offset = 0
    for p in model.parameters():                     # each gradient element = its position in the flat order (exact in float32 below 2^24)
        p.grad = torch.arange(offset, offset + p.numel(), dtype=torch.float32).reshape(p.shape)
        offset += p.numel()
    assert offset < 1 << 24
    total, norm = torch.tensor(3.25), torch.tensor(0.5)
    terms = [LossTerms(torch.arange(7, dtype=torch.float32))]
    a = bench.dump_outputs(str(tmp_path / 'a'), model, total, terms, norm)
    b = bench.dump_outputs(str(tmp_path / 'b'), model, total, terms, norm)
    on_disk = _dump_sizes(str(tmp_path / 'a'))
    for n in DUMP_NAMES:
        assert np.array_equal(a[n], b[n]) and np.array_equal(a[n], on_disk[n])
    assert a['loss'] == 3.25 and a['grad_norm'] == 0.5
    assert a['loss_terms'].shape == (1, 7) and np.array_equal(a['loss_terms'][0], np.arange(7))
    flat_p = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    assert a['params_sample'].shape == (bench.DUMP_SAMPLE,) and bench.DUMP_SAMPLE < flat_p.size
    pos = a['grads_sample'].astype(np.int64)
    assert np.all(np.diff(pos) > 0) and pos[0] < 0.1 * offset and pos[-1] > 0.9 * offset     # distinct, sorted, over the whole model
    assert np.array_equal(a['params_sample'], flat_p[pos])


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--steps must be at least 1' in r.stderr


@pytest.mark.gpu
def test_bench_steps_ms_per_step_and_dump(tmp_path):
    """The real timed path, briefly: the JSON line reports the requested step count and ms_per_step, and the dump holds a finite
    loss, its 7 terms and the samples of a model that was updated."""
    out = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--no-extras',
                        '--no-cpu-baseline', '--dump-outputs', out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res['steps'] == 3 and res['warmup'] == 1 and res['ms_per_step'] > 0
    a = _dump_sizes(out)
    assert a['loss'].shape == () and np.isfinite(a['loss']) and a['loss'] > 0
    assert a['loss_terms'].shape == (1, 7) and np.isfinite(a['loss_terms']).all()
    assert np.isfinite(a['grad_norm']) and a['grad_norm'] > 0
    assert np.isfinite(a['params_sample']).all() and np.isfinite(a['grads_sample']).all() and np.any(a['grads_sample'] != 0)


FULL_ONLY = ('sustained', 'f32_mode', 'inference_c4', 'cpu_baseline', 'roofline', 'roofline_hbm', 'parity')


def test_full_is_offered():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and '--full' in r.stdout


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only():
    """Without --full the run times its steps and prints the headline: none of the measurements that take runs of their own."""
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res['metric'] == 'mel frames/sec (fwd+bwd)' and res['unit'] == 'valid mel frames/s' and res['higher_is_better'] is True
    assert res['dtype'] == 'bf16' and res['steps'] == 2 and res['warmup'] == 1 and res['ms_per_step'] > 0 and res['value'] > 0
    assert not [k for k in FULL_ONLY if k in res]
