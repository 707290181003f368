"""The host side of the fine-tuning data (no GPU): pair discovery, shuffle and split against the reference's manifest, the rejection
rules, the order as a function of (seed, step), the restated start draw, and ``HiFiGanFineTuner.fit``'s accounting on a stub tuner."""
import os

import numpy as np
import pytest
import torch

from tests import finetune_data_helpers as fh
from ubisoft_laforge_daft_exprt_amd.vocoder_data import HiFiGanFineTuneData, find_pairs, pass_seed
from ubisoft_laforge_daft_exprt_amd.vocoder_finetune import HiFiGanFineTuner

OPTS = dict(segment_size=fh.SEGMENT, batch_size=4, device='cpu')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return fh.write_tree(str(tmp_path_factory.mktemp('finetune_tree')))


@pytest.fixture(scope='module')
def data(tree):
    return HiFiGanFineTuneData(tree, **OPTS)


def test_pairs_shuffle_and_split_equal_the_reference(tree, data):
    man = fh.manifest()
    rel = lambda p: os.path.relpath(p, tree).replace(os.sep, '/')
    found = find_pairs(tree)
    assert len(found) == 23 and [rel(w) for _, w in found] == sorted(man['pairs'])
    assert all(m[:-4] == w[:-4] and m.endswith('.npy') for m, w in found)
    assert [rel(p) for p in data.names] == man['pairs']
    assert [rel(p) for p in data.train_names] == man['train'] and [rel(p) for p in data.val_names] == man['val']
    assert [data.names[i] for i in data.train_indices] == data.train_names and len(data.val_indices) == max(1, int(23 * 0.1))
    lengths = {stem + '.wav': (T, n) for stem, T, n, _ in fh.CORPUS}
    assert [(data.mel_lengths[u], data.wav_lengths[u]) for u in range(23)] == [lengths[rel(p)] for p in data.names]
    # the resident size: int16 samples padded to 8 per utterance, fp32 mels, two int64 and two int32 table entries per utterance
    assert data.nbytes == sum((n + 7) // 8 * 8 * 2 + 80 * T * 4 for _, T, n, _ in fh.CORPUS) + 23 * 24
    # the same corpus from memory, in the data set's order, is the same object
    names, mels, wavs = fh.arrays([rel(p)[:-4] for p in data.names])
    again = HiFiGanFineTuneData.from_arrays(names, mels, wavs, **OPTS)
    assert again.train_indices == data.train_indices and again.val_indices == data.val_indices and again.nbytes == data.nbytes
    with pytest.raises(RuntimeError, match='GPU'):
        data.batch(0)


def _one(tmp_path, T, n, **wav):
    root = str(tmp_path)
    fh.write_tree(root, fh.CORPUS[:6])
    mel, pcm = fh.utterance('bad', T, n)
    np.save(os.path.join(root, 'bad.npy'), mel)
    fh.write_wav(os.path.join(root, 'bad.wav'), pcm, **wav)
    return root


def test_every_rejection_names_the_file(tmp_path, tree):
    empty = tmp_path / 'empty'
    empty.mkdir()
    with pytest.raises(RuntimeError, match='No mel/wav pairs'):
        HiFiGanFineTuneData(str(empty), **OPTS)
    # T_mel - fps - 1 < 0 for audio that reaches the segment; audio shorter than (T_mel - 1) * hop
    with pytest.raises(ValueError, match=r'bad\.wav.*randint'):
        HiFiGanFineTuneData(_one(tmp_path / 'few_frames', 8, 2048), **OPTS)
    with pytest.raises(ValueError, match=r'bad\.wav.*short'):
        HiFiGanFineTuneData(_one(tmp_path / 'short_audio', 12, 11 * 256 - 1), **OPTS)
    HiFiGanFineTuneData(_one(tmp_path / 'just_enough', 12, 11 * 256), **OPTS)
    # wav formats
    with pytest.raises(ValueError, match=r'bad\.wav.*sample rate 16000'):
        HiFiGanFineTuneData(_one(tmp_path / 'rate', 12, 3000, sr=16000), **OPTS)
    with pytest.raises(ValueError, match=r'bad\.wav.*2 channel'):
        HiFiGanFineTuneData(_one(tmp_path / 'stereo', 12, 3000, channels=2), **OPTS)
    with pytest.raises(ValueError, match=r'bad\.wav.*8 bits'):
        HiFiGanFineTuneData(_one(tmp_path / 'bytes', 12, 3000, width=1), **OPTS)
    root = _one(tmp_path / 'mel_shape', 12, 3000)
    np.save(os.path.join(root, 'bad.npy'), np.zeros((40, 12), dtype=np.float32))
    with pytest.raises(ValueError, match=r'bad\.npy.*\(40, 12\)'):
        HiFiGanFineTuneData(root, **OPTS)
    # 21 training pairs do not fill a batch of 22; the corpus is larger than max_bytes
    with pytest.raises(ValueError, match='21 training pairs'):
        HiFiGanFineTuneData(tree, **dict(OPTS, batch_size=22))
    HiFiGanFineTuneData(tree, **dict(OPTS, batch_size=21))
    full = HiFiGanFineTuneData(tree, **OPTS).nbytes
    with pytest.raises(ValueError, match='max_bytes'):
        HiFiGanFineTuneData(tree, max_bytes=full - 1, **OPTS)
    assert HiFiGanFineTuneData(tree, max_bytes=full, **OPTS).nbytes == full


def test_order_is_a_function_of_seed_and_step(tree, data):
    assert data.steps_per_epoch == 21 // 4 == 5 and data.fps == 8
    assert [data.epoch_of(s) for s in (0, 4, 5, 9, 10, 52)] == [(0, 0), (0, 4), (1, 0), (1, 4), (2, 0), (10, 2)]
    twin = HiFiGanFineTuneData(tree, **OPTS)
    other = HiFiGanFineTuneData(tree, seed=1, **OPTS)
    for e in range(4):
        order = data.epoch_order(e)
        assert order.dtype == torch.int32 and sorted(order.tolist()) == sorted(data.train_indices)
        assert torch.equal(order, twin.epoch_order(e)) and torch.equal(order, data.epoch_order(e))
        assert not torch.equal(order, other.epoch_order(e))
        assert not torch.equal(order, data.epoch_order(e + 1))
    assert other.train_indices == data.train_indices                  # the split is the reference's, whatever the seed
    assert len({pass_seed(s, e) for s in range(8) for e in range(8)}) == 64 and all(0 <= pass_seed(s, 3) < 1 << 63 for s in (0, 2 ** 64 - 1))


def test_restated_draw_stays_in_the_references_range():
    counters = np.arange(100_000, dtype=np.uint64)
    for seed, n in ((0, 1), (1, 2), (2, 3), (3, 52), (2 ** 64 - 1, 1000), (5, 2 ** 31 - 1)):
        for base in (0, 7 << 20, 1 << 63):                            # step 0, step 7, the validation stream
            s = fh.draw_start(seed, counters | np.uint64(base), n)
            assert s.min() >= 0 and s.max() <= n - 1, (seed, n, base)  # n = T - fps: [0, T - fps - 1]
            if n <= 52:
                assert s.min() == 0 and s.max() == n - 1 and len(np.unique(s)) == n
    # the streams differ: another step, the validation tag, another seed
    a = fh.draw_start(0, counters, 1000)
    assert (a != fh.draw_start(0, counters | np.uint64(1 << 20), 1000)).mean() > 0.99
    assert (a != fh.draw_start(0, counters | np.uint64(1 << 63), 1000)).mean() > 0.99
    assert (a != fh.draw_start(1, counters, 1000)).mean() > 0.99


def test_host_item_restatement_equals_the_reference_items():
    fx, rows = fh.fixture(), {r[0]: r for r in fh.CORPUS}
    for k, (stem, start) in enumerate(fh.ITEMS):
        mel, pcm = fh.utterance(*rows[stem])
        x, y = fh.host_item(mel, pcm, start)
        assert np.array_equal(x, fx[f'{k}/mel']) and np.array_equal(y, fx[f'{k}/audio']), stem
        fh.assert_mel_within_frontend_bar(stem, fh.host_loss_mel(y).numpy(), fx[f'{k}/mel_loss'], y)


class _StubData:
    steps_per_epoch = 4

    def batch(self, step):
        return ('x', 'y', 'y_mel', 'starts', step)

    def val_batches(self):
        return 'val'


class _StubTuner:
    fit = HiFiGanFineTuner.fit

    def __init__(self, step=0, epoch=0):
        self.step, self.epoch, self.calls = step, epoch, []

    def train_step(self, x, y, y_mel):
        assert (x, y, y_mel) == ('x', 'y', 'y_mel')
        self.step += 1
        self.calls.append(('step', self.step))
        return {'loss_mel': float(self.step)}

    def end_epoch(self):
        self.epoch += 1
        self.calls.append(('end_epoch', self.step))

    def validate(self, batches):
        assert batches == 'val'
        self.calls.append(('validate', self.step))
        return 0.5 + self.step

    def save_checkpoint(self, output_dir, save_disc=False):
        self.calls.append(('save', self.step, output_dir, save_disc, self.epoch))


def _of(calls, kind):
    return [c[1] for c in calls if c[0] == kind]


def test_fit_accounting_on_a_stub_tuner():
    data = _StubData()
    t = _StubTuner()
    r = t.fit(data, 0, output_dir='out')
    assert (r.steps, r.losses, r.validation) == (0, None, {}) and t.calls == [('save', 0, 'out', False, 0)]      # no step, no pass: the final save only
    t = _StubTuner()
    r = t.fit(data, 4, validation_interval=0, checkpoint_interval=0)
    assert r.steps == 4 and _of(t.calls, 'end_epoch') == [4] and t.epoch == 1 and not _of(t.calls, 'save') and r.losses == {'loss_mel': 4.0}
    t = _StubTuner()
    r = t.fit(data, 5, validation_interval=0, checkpoint_interval=0)
    assert _of(t.calls, 'end_epoch') == [4, 5] and t.epoch == 2       # one pass, and the partial one closed at the end
    # intervals, the final save, and the order at a boundary and at the end
    t, seen = _StubTuner(), []
    r = t.fit(data, 10, output_dir='out', validation_interval=3, checkpoint_interval=4, save_disc=True, log=lambda s, l: seen.append((s, l['loss_mel'])))
    assert r.steps == 10 and seen == [(s, float(s)) for s in range(1, 11)]
    assert _of(t.calls, 'validate') == [3, 6, 9] and r.validation == {3: 3.5, 6: 6.5, 9: 9.5}
    saves = [c for c in t.calls if c[0] == 'save']
    assert saves == [('save', 4, 'out', True, 1), ('save', 8, 'out', True, 2), ('save', 10, 'out', True, 2)]   # epoch: the completed passes
    assert _of(t.calls, 'end_epoch') == [4, 8, 10] and t.calls[-2:] == [('save', 10, 'out', True, 2), ('end_epoch', 10)]
    assert t.calls.index(('end_epoch', 4)) < t.calls.index(('save', 4, 'out', True, 1))
    # a final step that is a checkpoint step is saved once; without an output_dir nothing is saved
    t = _StubTuner()
    t.fit(data, 8, output_dir='out', validation_interval=0, checkpoint_interval=4)
    assert _of(t.calls, 'save') == [4, 8] and _of(t.calls, 'end_epoch') == [4, 8]
    t = _StubTuner()
    t.fit(data, 8, validation_interval=0, checkpoint_interval=4)
    assert not _of(t.calls, 'save')
    # a resumed tuner goes on from its step: the rest of the pass, then the boundary
    t = _StubTuner(step=2, epoch=0)
    r = t.fit(data, 4, validation_interval=0, checkpoint_interval=0)
    assert r.steps == 2 and _of(t.calls, 'step') == [3, 4] and _of(t.calls, 'end_epoch') == [4] and t.epoch == 1
