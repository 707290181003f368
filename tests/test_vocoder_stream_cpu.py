"""CPU checks of the streaming vocoder's host side: the plan's lags and rings by interval bookkeeping, the plan's schedule run in
float64 on ring buffers against the plain-torch generator, and argument validation."""
import pytest
import torch

from tests import vocoder_helpers as vh
from tests import vocoder_torch
from tests.vocoder_stream_helpers import emulate, simulate
from ubisoft_laforge_daft_exprt_amd import vocoder as voc

CHUNKS = (1, 3, 8, 32)
LENGTHS = (1, 13, 14, 65, 300)


@pytest.mark.parametrize('chunk_frames', CHUNKS)
def test_plan_bookkeeping(chunk_frames):
    plan = voc.stream_plan(None, chunk_frames)
    assert 13 <= plan.lookahead <= 14                  # the measured right reach is 3256 samples = ceil 13 frames; one frame of rounding slack
    kinds = [ln['kind'] for ln in plan.launches]
    assert len(plan.launches) == 60 and kinds.count('pair') == 18 and kinds[-1] == 'post'
    for name, t in plan.tensors.items():
        assert t['ring'] & (t['ring'] - 1) == 0 and t['ring'] >= chunk_frames * t['scale'] + t['lag'], name
    for ln in plan.launches:
        if ln['up'] > 1:
            assert plan.tensors[ln['y']]['lag'] % ln['up'] == 0
    sums = [plan.tensors[f'sum.{i}']['lag'] for i in range(4)]
    assert sums[3] == 3                                # conv_post's right reach
    for length in LENGTHS:
        simulate(plan, length)


def test_ring_sizes_do_not_depend_on_the_length_and_grow_with_the_chunk():
    a, b = voc.stream_plan(None, 8), voc.stream_plan(voc.v1_config(), 8)
    assert {n: t['ring'] for n, t in a.tensors.items()} == {n: t['ring'] for n, t in b.tensors.items()}
    assert a.ring_bytes(3) == 3 * a.ring_bytes(1)
    assert voc.stream_plan(None, 32).ring_bytes() > a.ring_bytes()
    lags = {n: t['lag'] for n, t in a.tensors.items()}
    assert lags == {n: t['lag'] for n, t in voc.stream_plan(None, 32).tensors.items()}        # lags belong to the network, not the chunk


# ---- the schedule in float64 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def weights64():
    folded = voc.fold_state_dict(vh.state_dict(), voc.HiFiGANGenerator().layer_names())
    return vocoder_torch.to(folded, 'cpu', torch.float64)


@pytest.fixture(scope='module')
def reference64(weights64):
    g = torch.Generator().manual_seed(9)
    mel = (torch.randn(1, 80, 41, generator=g, dtype=torch.float64) * 1.5 - 5.0).clamp(-11.5, 2.0)
    with torch.no_grad():
        return mel, {n: vocoder_torch.generator(mel[:, :, :n], weights64)[0] for n in (14, 41)}


@pytest.mark.parametrize('chunk_frames', [3, 8])
@pytest.mark.parametrize('length', [14, 41])
def test_schedule_in_float64_equals_the_whole_generator(weights64, reference64, length, chunk_frames):
    mel, refs = reference64
    plan = voc.stream_plan(None, chunk_frames)
    with torch.no_grad():
        got = emulate(plan, mel[:, :, :length], length, weights64)
    ref = refs[length]
    assert got.shape[0] == -(-length // chunk_frames) * chunk_frames * voc.HOP
    err = (got[:ref.shape[0]] - ref).abs().max().item()
    print(f'length {length}, chunks of {chunk_frames}: max abs {err:.2e}')
    assert err <= 1e-12
    assert torch.count_nonzero(got[ref.shape[0]:]).item() == 0


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_stream_argument_errors_and_the_cpu_device_error():
    with pytest.raises(ValueError, match='chunk_frames'):
        voc.stream_plan(None, 0)
    with pytest.raises(NotImplementedError):
        voc.stream_plan(dict(voc.v1_config(), upsample_rates=[8, 8, 4, 2]), 8)
    v = voc.HiFiGanVocoder(vh.state_dict(), device='cpu')
    mels = torch.zeros(2, 80, 5)
    with pytest.raises(ValueError, match='chunk_frames'):
        v.stream(mels, [5, 3], chunk_frames=0)
    with pytest.raises(ValueError, match='mels must be'):
        v.stream(torch.zeros(2, 79, 5), [5, 3])
    with pytest.raises(ValueError, match='lengths'):
        v.stream(mels, [5])
    with pytest.raises(RuntimeError, match='GPU'):
        v.stream(mels, [5, 3])


def test_window_launches_are_priced_by_the_rows_of_one_window():
    from ubisoft_laforge_daft_exprt_amd import profiling
    geom = profiling.Geometry([[5, 9, 12]])
    a = dict(B=3, N=96, in_scale=8, Cin=512, Cout=256, taps=2, up=8, bf16=1, R=0, acc_mode=0, step=32, lag=10)
    label, bound, flops, byt = profiling.price('dx_voc_conv_win', a, geom)
    assert (label, bound) == ('voc_ups<bf16>', 'mfma') and flops == 2.0 * 2 * 512 * 256 * (3 * 32 * 8)
    assert byt == 3 * 32 * 512 * 4 + 3 * 32 * 8 * 256 * 4
    p = dict(B=3, N=96, scale=8, C=64, taps=7, bf16=0, acc_mode=1, step=32, lag=10)
    assert profiling.price('dx_voc_pair_win', p, geom)[2] == 2.0 * 2 * 7 * 64 * 64 * (3 * 32)
    assert profiling.price('dx_voc_stream_advance', {}, geom)[:2] == ('voc_stream_advance', 'hbm')


def test_window_entry_points_reject_bad_windows_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import lib, DxError
    conv = lambda **k: lib().dx_voc_conv_win(4096, 64 * 8, 64, 1, 1, None, 8192, 64 * 8, None, 64 * 8, 1, 1, 1, 8, 64, 64, 3, 1, 1, 1, 0, 0,
                                             k.get('cursor', 16), k.get('step', 4), 0, k.get('mx', 7), k.get('my', 7), 0, None)
    with pytest.raises(DxError, match='window'):
        conv(cursor=None)
    with pytest.raises(DxError, match='window'):
        conv(step=0)
    with pytest.raises(DxError, match='window'):
        conv(mx=6)                                     # not 2^k - 1
    with pytest.raises(DxError, match='ring'):
        conv(my=15)                                    # 16 rows of 64 do not fit a batch stride of 8 rows
    with pytest.raises(DxError, match='ring'):
        lib().dx_voc_pair_win(4096, 64 * 8, 1, 1, 1, 1, 8192, 64 * 8, 1, 1, 1, 8, 64, 3, 1, 0, 0, 16, 4, 0, 15, 7, None)
    with pytest.raises(DxError, match='chunk buffer'):
        lib().dx_voc_post_win(4096, 32 * 8, 1, 1, 8192, 8, 1, 1, 1, 8, 8, 16, 4, 0, 7, 7, None)
    with pytest.raises(DxError, match='null'):
        lib().dx_voc_stream_advance(None, None)
