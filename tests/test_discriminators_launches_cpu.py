"""CPU checks of the one layer table every discriminator walk runs from (``discriminators.layer_table``): every library call of the
module forwards, ``losses``, ``generator_loss_grad`` and ``discriminator_loss_grad`` against the sequence recorded from the code before the
walks shared the table (tests/golden/make_golden_discriminators_launches.py), and the table's map shapes against the reference fixture."""
import importlib.util
import json
import os

import pytest

from tests import disc_helpers as dh
from ubisoft_laforge_daft_exprt_amd import discriminators as disc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [(T, precision) for T in (12, 257) for precision in ('f32', 'bf16')]
ENTRIES = ('forward_mpd', 'forward_msd', 'losses', 'losses_again', 'generator_loss_grad', 'generator_loss_grad_again')
F32_ENTRIES = ('discriminator_loss_grad', 'discriminator_loss_grad_folded', 'losses_after_refresh_folded')
# at either length: 38 layers have a pack (two calls each to build one), 8 + 38 + 8 layer launches, 2 pools, the losses
COUNTS = {'losses': 38 + 38 + 8 + 38 + 8 + 2 + 1 + 1, 'losses_again': 57, 'generator_loss_grad': 189, 'discriminator_loss_grad': 227,
          'discriminator_loss_grad_folded': 149}


@pytest.fixture(scope='module')
def recorder():
    spec = importlib.util.spec_from_file_location('make_golden_discriminators_launches',
                                                  os.path.join(GOLDEN, 'make_golden_discriminators_launches.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(GOLDEN, 'discriminators_launches.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def again(recorder):
    """One recording per case for the whole module, through JSON as the fixture went."""
    made = {}

    def get(T, precision):
        if (T, precision) not in made:
            made[T, precision] = json.loads(json.dumps(recorder.record(T, precision)))
        return made[T, precision]
    return get


@pytest.mark.parametrize('T,precision', CASES)
def test_every_library_call_equals_the_recorded_sequence(recorder, again, recorded, T, precision):
    """What the file writes out (recorder.FULL) is compared call by call; of every other entry it holds the digest."""
    want, got = recorded[f'T{T}-{precision}'], again(T, precision)
    assert list(got) == list(want) == list(ENTRIES + (F32_ENTRIES if precision == 'f32' else ()))
    assert all(isinstance(calls, list) == (entry in recorder.FULL.get(f'T{T}-{precision}', ())) for entry, calls in want.items())
    for entry in want:
        if isinstance(want[entry], dict):
            assert recorder.digest(got[entry]) == want[entry], entry
            continue
        assert len(got[entry]) == len(want[entry]), entry
        for i, (g, w) in enumerate(zip(got[entry], want[entry])):
            assert g == w, (entry, i)


@pytest.mark.parametrize('T,precision', CASES)
def test_call_counts_and_a_repeated_call_builds_nothing(again, T, precision):
    got = again(T, precision)
    for entry, n in COUNTS.items():
        if entry in got:
            assert len(got[entry]) == n, entry
    for entry in ('losses_again', 'generator_loss_grad_again'):
        assert not [c[0] for c in got[entry] if c[0].endswith(('_pack', '_size', '_workspace'))], entry
        first = got[entry[:-len('_again')]]
        launches = [c for c in first if not c[0].endswith(('_pack', '_pack_size', '_size', '_workspace'))]
        # the same launches on the same buffers in the same order; only what a call allocates itself (the stacked waveforms, the
        # losses, dy_hat) is new, and no hidden-layer launch touches those
        assert [c[0] for c in launches] == [c[0] for c in got[entry]]
        for kind in ('dx_disc_conv', 'dx_disc_post', 'dx_disc_conv_dgrad'):
            assert [c for c in launches if c[0] == kind] == [c for c in got[entry] if c[0] == kind], (entry, kind)


def test_two_recordings_in_one_process_are_equal(recorder, again):
    assert json.loads(json.dumps(recorder.record(12, 'f32'))) == again(12, 'f32')          # no address leaked into a name


@pytest.mark.parametrize('T', (12, 257))
def test_refreshed_packs_are_built_from_the_tensors_handed_in(again, T):
    calls = again(T, 'f32')['losses_after_refresh_folded']
    packs = [c for c in calls if c[0] == 'dx_disc_pack']
    assert len(packs) == 38 and len(calls) == 2 * 38 + 57
    assert sum(c[1].startswith('folded:') and c[1].endswith('.w+0') for c in packs) == 32      # the spectral sub-discriminator folds its own six
    assert not [c for c in packs if c[1].startswith(('mpd.', 'msd.'))]
    firsts = [c for c in calls if c[0] == 'dx_disc_first']
    assert sum(c[4].startswith('folded:') and c[5].startswith('folded:') for c in firsts) == 7


@pytest.mark.parametrize('T', dh.LENGTHS)
def test_layer_table_has_the_reference_map_shapes(T):
    """The table's lengths and channel counts against the feature-map shapes the reference fixture stores, (B, C, H, p) and (B, C, N)."""
    z = dh.fixture()
    lengths = [T, T // 2 + 1, (T // 2 + 1) // 2 + 1]
    for d, i, j in dh.fmap_keys(T):
        p = disc.PERIODS[i] if d == 'mpd' else 1
        table = disc.layer_table(disc.MPD_LAYERS if d == 'mpd' else disc.MSD_LAYERS, T if d == 'mpd' else lengths[i], p)
        assert table is disc.layer_table(disc.MPD_LAYERS if d == 'mpd' else disc.MSD_LAYERS, T if d == 'mpd' else lengths[i], p)
        assert [ly.name for ly in table] == [f'convs.{k}' for k in range(len(table) - 1)] + ['conv_post']
        ly = table[j]
        want = [dh.BATCH, ly.cout, ly.n_out] + ([p] if d == 'mpd' else [])
        assert list(z[f'{T}/{d}/{i}/fmap{j}/shape']) == want, (d, i, j)
        assert ly.n_in == (-(-lengths[0 if d == 'mpd' else i] // p) if j == 0 else table[j - 1].n_out) and ly.cin == (1 if j == 0 else table[j - 1].cout)
        # a map is (rows, n, p, c) channels-last and a kernel row one column of one batch row: batch, column and position strides
        assert ly.p == p and ly.strides('out') == (ly.n_out * p * ly.cout, ly.cout, p * ly.cout)
        assert ly.strides('in') == (ly.n_in * p * ly.cin, ly.cin, p * ly.cin)
