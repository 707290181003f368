"""The fine-tuning data on the GPU: ``dx_ft_batch`` against the reference's items (bitwise: the conversion is exact and the rest is a
copy), the loss mel against the existing front end and its bar, the step's order and draws against their host restatements, the
validation stream, the launch shapes (one row, an odd and a single chunk), and ``HiFiGanFineTuner.fit`` with its bitwise resume."""
import os

import numpy as np
import pytest
import torch

from tests import finetune_data_helpers as fh
from ubisoft_laforge_daft_exprt_amd import mel
from ubisoft_laforge_daft_exprt_amd.vocoder_data import VAL_TAG, HiFiGanFineTuneData

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
ROWS = {r[0]: r for r in fh.CORPUS}


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    """The 23-pair tree read from disk: 21 training pairs in batches of 4 (5 steps per pass), 2 validation pairs."""
    root = fh.write_tree(str(tmp_path_factory.mktemp('finetune_tree')))
    return HiFiGanFineTuneData(root, segment_size=fh.SEGMENT, batch_size=4, seed=7, device=DEV)


def _stem(data, utt):
    name = data.names[utt].replace(os.sep, '/')
    name = name[:-4] if name.endswith('.wav') else name
    return next(s for s in ROWS if name == s or name.endswith('/' + s))


_UTTERANCES = {}


def _host_rows(data, utts, starts):
    """The reference's per-item path restated on the host for these rows -> (x (B, 80, fps), y (B, segment))."""
    items = []
    for u, s in zip(utts, starts):
        stem = _stem(data, u)
        if stem not in _UTTERANCES:
            _UTTERANCES[stem] = fh.utterance(*ROWS[stem])
        items.append(fh.host_item(*_UTTERANCES[stem], s))
    return np.stack([x for x, _ in items]), np.stack([y for _, y in items])


def test_assemble_equals_the_reference_items_bitwise(data):
    fx = fh.fixture()
    utts = [next(u for u in range(len(data.names)) if _stem(data, u) == stem) for stem, _ in fh.ITEMS]
    starts = [s for _, s in fh.ITEMS]
    x, y, y_mel, starts_out, utts_out = data.assemble(utts, starts)
    assert x.shape == (len(utts), 80, fh.FPS) and y.shape == (len(utts), fh.SEGMENT) and y_mel.shape == x.shape
    assert starts_out.tolist() == starts and utts_out.tolist() == utts and starts_out.dtype == utts_out.dtype == torch.int32
    want = mel.mel_spectrogram(y, 1024, 80, fh.SR, fh.HOP, 1024, 0, None, center=False)
    assert torch.equal(y_mel, want)
    for k, (stem, start) in enumerate(fh.ITEMS):
        assert np.array_equal(x[k].cpu().numpy(), fx[f'{k}/mel']), (stem, start)
        assert np.array_equal(y[k].cpu().numpy(), fx[f'{k}/audio']), (stem, start)
        fh.assert_mel_within_frontend_bar(f'{stem}@{start}', y_mel[k].cpu().numpy(), fx[f'{k}/mel_loss'], fx[f'{k}/audio'])
    with pytest.raises(ValueError, match='start'):
        data.assemble([utts[0]], [60 - fh.FPS])                        # one past the reference's largest start
    with pytest.raises(ValueError, match='start'):
        data.assemble([utts[4]], [1])                                  # a short utterance starts at 0


def test_batch_follows_the_order_and_the_draw(data):
    assert data.steps_per_epoch == 5
    for step in (0, 4, 5, 11):                                        # 4 | 5: the two sides of a pass boundary
        x, y, y_mel, starts, utts = data.batch(step)
        epoch, pos = data.epoch_of(step)
        assert utts.tolist() == data.epoch_order(epoch)[4 * pos:4 * pos + 4].tolist(), step
        assert starts.tolist() == fh.expected_starts(data, step, utts.tolist()), step
        assert all(0 <= s <= data.max_start(u) for s, u in zip(starts.tolist(), utts.tolist()))
        for b in range(4):                                             # a row of the batch is bitwise the row assembled alone
            xa, ya, ma, _, _ = data.assemble([int(utts[b])], [int(starts[b])])
            assert torch.equal(x[b], xa[0]) and torch.equal(y[b], ya[0]) and torch.equal(y_mel[b], ma[0]), (step, b)
        hx, hy = _host_rows(data, utts.tolist(), starts.tolist())
        assert np.array_equal(x.cpu().numpy(), hx) and np.array_equal(y.cpu().numpy(), hy), step
        again = data.batch(step)
        assert all(torch.equal(a, b) for a, b in zip((x, y, y_mel, starts, utts), again)), step
    assert data.batch(4)[4].tolist() == data.epoch_order(0)[16:20].tolist() and data.batch(5)[4].tolist() == data.epoch_order(1)[:4].tolist()
    assert not torch.equal(data.epoch_order(0), data.epoch_order(1))


def test_validation_batches_cover_every_utterance_with_fixed_crops():
    names, mels, wavs = fh.arrays([r[0] for r in fh.CORPUS])
    data = HiFiGanFineTuneData.from_arrays(names, mels, wavs, segment_size=fh.SEGMENT, val_split=0.3, batch_size=4, seed=3, device=DEV)
    assert len(data.val_indices) == 6
    first = list(data.val_batches())
    assert [x.shape[0] for x, _ in first] == [4, 2] and all(x.shape[1:] == (80, fh.FPS) and m.shape == x.shape for x, m in first)
    starts = []
    for u in data.val_indices:
        n = data.mel_lengths[u] - data.fps
        starts.append(0 if data.wav_lengths[u] < fh.SEGMENT else int(fh.draw_start(3, np.uint64(VAL_TAG | u), n)))
    hx, hy = _host_rows(data, data.val_indices, starts)                # row i is validation utterance i: each exactly once, in order
    assert np.array_equal(torch.cat([x for x, _ in first]).cpu().numpy(), hx)
    want = mel.mel_spectrogram(torch.from_numpy(hy).to(DEV), 1024, 80, fh.SR, fh.HOP, 1024, 0, None, center=False)
    assert torch.equal(torch.cat([m for _, m in first]), want)
    data.batch(0)                                                      # training draws in between change nothing
    second = list(data.val_batches())
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(first, second))


@pytest.mark.parametrize('B', [1, 400, 1100])
def test_one_row_odd_and_single_chunk_launches(data, B):
    """Rows of 256 + 640 work items: 4 workgroups per row up to B = 256, then ceil(1024 / B): 3 at B = 400, 1 at B = 1100."""
    g = np.random.default_rng(B)
    utts = [int(u) for u in g.integers(0, len(data.names), B)]
    starts = [int(g.integers(0, data.max_start(u) + 1)) for u in utts]
    x, y, y_mel, starts_out, utts_out = data.assemble(utts, starts)
    assert starts_out.tolist() == starts and utts_out.tolist() == utts
    hx, hy = _host_rows(data, utts, starts)
    assert np.array_equal(x.cpu().numpy(), hx) and np.array_equal(y.cpu().numpy(), hy)
    xa, ya, ma, _, _ = data.assemble(utts[-1:], starts[-1:])
    assert torch.equal(x[-1], xa[0]) and torch.equal(y[-1], ya[0]) and torch.equal(y_mel[-1], ma[0])


def test_entry_point_rejects_bad_arguments(data):
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    wav, wav_off, wav_len, mels, mel_off, mel_len = (t.data_ptr() for t in data._tables)
    x, y = torch.empty(1, 80, 8, device=DEV), torch.empty(1, 2048, device=DEV)
    order = data._order(0)
    call = lambda **kw: lib().dx_ft_batch(*{**dict(wav=wav, wav_off=wav_off, wav_len=wav_len, mel=mels, mel_off=mel_off, mel_len=mel_len,
                                                   n_utt=23, utts=None, order=order.data_ptr(), order_pos=0, n_order=21, starts_in=None, seed=0,
                                                   counter=0, by_utt=0, x=x.data_ptr(), y=y.data_ptr(), starts_out=None, utts_out=None, B=1,
                                                   segment_size=2048, hop_size=256, fps=8, n_mels=80, stream=None), **kw}.values())
    for bad, match in ((dict(wav=None), 'null'), (dict(order=None), 'null'), (dict(B=0), 'bad sizes'), (dict(fps=7), 'whole hops'),
                       (dict(segment_size=2040), 'whole hops'), (dict(wav=wav + 2), 'aligned'), (dict(order_pos=21), 'outside the order')):
        with pytest.raises(DxError, match=match):
            call(**bad)


class _Loop:
    """B = 2, a 6-utterance training set (3 steps per pass) and one validation utterance; the V3 generator and the seeded
    discriminators of the fine-tuner tests.  Built once: leave it unchanged."""

    def __init__(self, tmp):
        stems = ['a/utt00', 'a/utt01', 'a/utt02', 'a/utt03', 'a/deep/utt04', 'a/deep/utt05', 'a/deep/utt06']
        self.data = HiFiGanFineTuneData.from_arrays(*fh.arrays(stems), segment_size=fh.SEGMENT, batch_size=2, seed=11, device=DEV)
        assert self.data.steps_per_epoch == 3 and len(self.data.val_indices) == 1
        straight = fh.tuner(DEV)
        self.val_before = straight.validate(self.data.val_batches())
        self.before, _ = fh.tuner_state(straight)
        self.params = fh.parameter_keys(straight)
        self.logged = []
        self.result = straight.fit(self.data, 3, validation_interval=3, log=lambda step, losses: self.logged.append((step, losses)))
        torch.cuda.synchronize()
        self.after, self.counters = fh.tuner_state(straight)
        self.val_after = straight.validate(self.data.val_batches())
        # the same three steps by hand
        by_hand = fh.tuner(DEV)
        self.hand_losses = [dict(by_hand.train_step(*self.data.batch(s)[:3]).items()) for s in range(3)]
        # two steps, the checkpoint fit writes, a new tuner from its two files, the third step
        first = fh.tuner(DEV)
        first.fit(self.data, 2, output_dir=tmp, validation_interval=0, save_disc=True)
        self.first_counters = (first.step, first.epoch)
        del first
        self.files = sorted(os.listdir(tmp))
        resumed = fh.tuner(DEV, os.path.join(tmp, 'g_00000002'), os.path.join(tmp, 'do_00000002'))
        self.restored_counters = (resumed.step, resumed.epoch, resumed.optim_g.lr)
        self.resumed_result = resumed.fit(self.data, 3, validation_interval=0)
        torch.cuda.synchronize()
        self.resumed, self.resumed_counters = fh.tuner_state(resumed)


@pytest.fixture(scope='module')
def loop(tmp_path_factory):
    return _Loop(str(tmp_path_factory.mktemp('finetune_fit')))


def test_fit_changes_every_parameter_and_equals_hand_made_steps(loop):
    assert loop.result.steps == 3 and [s for s, _ in loop.logged] == [1, 2, 3]
    assert loop.counters[:4] == (3, 1, 3, 3) and loop.counters[4] == loop.counters[5] == 2e-4 * 0.999      # one whole pass: one decay
    assert len(loop.params) == 154 + 69                                # as tests/test_finetune_gpu.py counts them (V3: 23 layers)
    for k in loop.params:
        assert not torch.equal(loop.before[k], loop.after[k]), f'{k} did not change'
    assert all(torch.isfinite(v).all() for v in loop.after.values())
    fit_losses = [dict(l.items()) for _, l in loop.logged]
    assert fit_losses == loop.hand_losses and dict(loop.result.losses.items()) == loop.hand_losses[2]
    assert len({l['loss_mel'] for l in fit_losses}) == 3 and all(np.isfinite(list(l.values())).all() for l in fit_losses)
    assert list(loop.result.validation) == [3] and loop.result.validation[3] == loop.val_after
    assert np.isfinite([loop.val_before, loop.val_after]).all() and loop.val_after != loop.val_before


def test_fit_resumes_bitwise_from_its_own_checkpoint(loop):
    assert loop.files == ['do_00000002', 'g_00000002']
    assert loop.first_counters == (2, 1)                               # the partial pass was closed, after the checkpoint was written
    assert loop.restored_counters == (2, 0, 2e-4)                      # ... which holds the completed passes: none
    assert loop.resumed_result.steps == 1
    assert loop.resumed_counters == loop.counters
    assert sorted(loop.resumed) == sorted(loop.after)
    for k in loop.after:
        assert torch.equal(loop.resumed[k], loop.after[k]), k
    assert dict(loop.resumed_result.losses.items()) == loop.hand_losses[2]
