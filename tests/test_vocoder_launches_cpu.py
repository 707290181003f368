"""CPU checks of the one launch list both vocoder paths run (``vocoder.generator_launches``): every library call of ``infer_batch`` and
``stream`` against the sequence recorded from the code before the two paths shared it, the whole call's reuse of its five workspace
slots by bookkeeping, and the launch counts."""
import importlib.util
import json
import os

import pytest

from ubisoft_laforge_daft_exprt_amd import vocoder as voc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [(name, precision) for name in ('v1', 'v2', 'v3') for precision in ('f32', 'bf16')]
COUNTS = {('v1', 'f32'): 60, ('v1', 'bf16'): 60, ('v2', 'f32'): 42, ('v2', 'bf16'): 42, ('v3', 'f32'): 23, ('v3', 'bf16'): 19}


@pytest.fixture(scope='module')
def recorder():
    spec = importlib.util.spec_from_file_location('make_golden_vocoder_launches', os.path.join(GOLDEN, 'make_golden_vocoder_launches.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(GOLDEN, 'vocoder_launches.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name,precision', CASES)
def test_every_library_call_equals_the_recorded_sequence(recorder, recorded, name, precision):
    want = recorded[f'{name}-{precision}']
    got = json.loads(json.dumps(recorder.record(name, precision)))          # through JSON, as the fixture went
    assert len(want['infer_batch']) == 2 * COUNTS[name, precision] and len(want['stream_step']) == COUNTS[name, precision] + 1
    assert got['stream_steps'] == want['stream_steps'] == 3
    for part in ('infer_batch', 'stream_step'):
        assert len(got[part]) == len(want[part]), part
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, (part, i)


@pytest.mark.parametrize('name,precision', CASES)
def test_whole_call_slots_never_hold_two_live_tensors(name, precision):
    generator = voc.generator_launches(voc.CONFIGS[name](), precision)
    slot = {n: t['slot'] for n, t in generator.tensors.items()}
    assert all(0 <= s < 5 for s in slot.values())

    def reads(ln):                        # the tensors a launch reads: x, the residual, and the output it accumulates into
        return {n for n in (ln['x'], ln['r'], ln['y'] if ln['acc'] else None) if n in slot}

    written = set()
    for i, ln in enumerate(generator.launches):
        x, y, r = ln['x'], ln['y'], ln['r']
        assert reads(ln) <= written, (i, 'reads a tensor no launch has written')
        if y not in slot:
            assert y == 'audio' and i == len(generator) - 1
            continue
        assert slot.get(x) != slot[y], (i, 'x and y share a slot: the kernels require X != Y')
        assert r is None or r == y or slot[r] != slot[y], (i, 'the residual sits in the slot the launch writes')
        if not ln['acc']:
            assert y not in written, (i, 'writes a tensor twice')
            evicted = {n for n in written if slot[n] == slot[y]}
            for later in generator.launches[i + 1:]:
                assert not (reads(later) & evicted), (i, later['layer'], 'reads a tensor that an earlier launch overwrote')
        written.add(y)


@pytest.mark.parametrize('name,precision', CASES)
def test_launch_counts_and_the_stream_plan_has_the_same_launches(name, precision):
    cfg = voc.CONFIGS[name]()
    generator = voc.generator_launches(cfg, precision)
    assert len(generator) == COUNTS[name, precision]
    assert generator is voc.generator_launches({k: tuple(v) if isinstance(v, list) and not isinstance(v[0], list) else v for k, v in cfg.items()}, precision)
    plan = voc.stream_plan(cfg, 4, precision)
    assert [(ln['kind'], ln['layer'], ln.get('layer2')) for ln in plan.launches] == [(ln['kind'], ln['layer'], ln.get('layer2')) for ln in generator.launches]
    for ln, planned in zip(generator.launches, plan.launches):
        assert 'lag' not in ln and 'step' not in ln                                  # the plan wrote into its own copies
        assert {k: v for k, v in planned.items() if k not in ('lag', 'step')} == ln
    assert all('ring' not in t for t in generator.tensors.values())
