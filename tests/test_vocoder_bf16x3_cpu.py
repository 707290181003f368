"""The vocoder's 'bf16x3' precision (split-bf16 operands, operand mode 2) without a GPU: the name, the launch lists and streaming plans
(the f32 ones, entry for entry), the pack sizes, and what the library refuses before any launch."""
import pytest
import torch

from tests import vocoder_helpers as vh
from ubisoft_laforge_daft_exprt_amd import vocoder as voc

CONFIGS = {'v1': voc.v1_config, 'v2': voc.v2_config, 'v3': voc.v3_config}


def test_the_name_is_accepted_everywhere_a_precision_is():
    assert voc.PRECISIONS == {'f32': 0, 'bf16': 1, 'bf16x3': 2}
    sd = vh.state_dict()
    v = voc.HiFiGanVocoder(sd, device='cpu', precision='bf16x3')
    assert v.precision == 'bf16x3' and v.generator is not None
    assert voc.load_hifigan_vocoder(sd, device='cpu', precision='bf16x3').precision == 'bf16x3'
    assert voc.HiFiGANGenerator(precision='bf16x3').precision == 'bf16x3'
    for name in vh.VARIANTS:
        w = voc.HiFiGanVocoder.from_checkpoint(vh.state_dict(name), device='cpu', precision='bf16x3')
        assert w.precision == 'bf16x3' and w.config == CONFIGS[name]()
    for bad in ('fp16', 'bf16x2', 'BF16X3'):
        with pytest.raises(ValueError, match='precision'):
            voc.HiFiGanVocoder(sd, device='cpu', precision=bad)
        with pytest.raises(ValueError, match='precision'):
            voc.generator_launches(None, bad)


@pytest.mark.parametrize('name,count', [('v1', 60), ('v2', 42), ('v3', 23)])
def test_launch_list_and_stream_plan_are_the_f32_ones(name, count):
    cfg = CONFIGS[name]()
    a, b = voc.generator_launches(cfg, 'f32'), voc.generator_launches(cfg, 'bf16x3')
    assert len(b) == len(a) == count
    assert b.launches == a.launches and b.tensors == a.tensors           # the precision is no field of a launch: the lists are equal
    assert not any(ln['kind'] == 'chain' for ln in b.launches)
    assert voc.HiFiGanVocoder(vh.state_dict(name), config=cfg, device='cpu', precision='bf16x3').topology.launches == a.launches
    for F in (1, 8, 32):
        p, q = voc.stream_plan(cfg, F, 'f32'), voc.stream_plan(cfg, F, 'bf16x3')
        assert q.launches == p.launches and q.tensors == p.tensors and q.lookahead == p.lookahead
        assert q.ring_bytes(1) == p.ring_bytes(1)
    if name == 'v1':
        assert round(voc.stream_plan(cfg, 32, 'bf16x3').ring_bytes(1) / 1e6) == 78


def _size(cout, cin, taps, up, mode):
    from ubisoft_laforge_daft_exprt_amd._lib import lib
    n = torch.zeros(1, dtype=torch.long)
    lib().dx_voc_pack_size(cout, cin, taps, up, mode, n.data_ptr())
    return int(n.item())


def test_pack_size_is_the_f32_packs():
    """A lane holds eight hi and eight lo bf16 per 32-deep k step: 32 bytes, what two 16-deep f32 steps hold.  So the pack is byte for
    byte the f32 pack's size whenever Cin is whole 32-deep steps -- every layer but conv_pre (Cin = 80) and V2's padded 16-channel
    stage, where the mode rounds Cin up to 32 as the bf16 mode does and the pack is the f32 pack's of that rounded Cin."""
    for cout, cin, taps, up in ((256, 512, 2, 8), (128, 256, 2, 8), (32, 64, 2, 2),       # transposed convs
                                (256, 256, 11, 1), (128, 128, 3, 1), (64, 64, 7, 1),
                                (16, 32, 2, 2), (16, 32, 3, 1)):                            # 16 columns
        assert _size(cout, cin, taps, up, 2) == _size(cout, cin, taps, up, 0) == 2 * _size(cout, cin, taps, up, 1), (cout, cin, taps, up)
    # conv_pre (80 -> 512, k 7): three 32-deep steps, the f32 pack's size at Cin = 96 (the f32 pack itself holds five 16-deep steps)
    assert _size(512, 80, 7, 1, 2) == _size(512, 96, 7, 1, 0) == 2 * _size(512, 80, 7, 1, 1) == 7 * 32 * 3 * 64 * 32
    assert _size(512, 80, 7, 1, 0) == 7 * 32 * 5 * 64 * 16
    # 16 -> 16 (V2's last stage): half a step, zero-padded
    assert _size(16, 16, 3, 1, 2) == _size(16, 32, 3, 1, 0) == 2 * _size(16, 16, 3, 1, 1)


def test_what_the_library_refuses_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import lib, DxError
    L = lib()
    chain = lambda mode: L.dx_voc_chain(4096, 64 * 8, 1, 1, 1, 1, 8192, 1, 1, 1, 8, 64, 3, 1, 2, 0, mode, None)
    with pytest.raises(DxError, match='no split-bf16 form'):
        chain(2)
    with pytest.raises(DxError, match='no split-bf16 form'):
        L.dx_voc_chain_win(4096, 64 * 8, 1, 1, 1, 1, 8192, 64 * 8, 1, 1, 1, 8, 64, 3, 1, 2, 0, 2, 16, 4, 0, 7, 7, None)
    with pytest.raises(DxError, match='bf16'):
        chain(3)
    conv = lambda mode: L.dx_voc_conv(4096, 64 * 8, 64, 1, 1, None, 8192, 64 * 8, None, 1, 1, 1, 8, 64, 64, 3, 1, 1, 1, 0, mode, None)
    pair = lambda mode: L.dx_voc_pair(4096, 64 * 8, 1, 1, 1, 1, 8192, 1, 1, 1, 8, 64, 3, 1, 0, mode, None)
    for mode in (3, -1):
        with pytest.raises(DxError, match='bf16'):
            conv(mode)
        with pytest.raises(DxError, match='bf16'):
            pair(mode)
        with pytest.raises(DxError, match='bad shape'):
            _size(64, 64, 3, 1, mode)
        with pytest.raises(DxError, match='bad shape'):
            L.dx_voc_pack(4096, 8192, 64, 64, 3, 1, mode, None)


def test_gradients_exist_for_f32_only():
    from ubisoft_laforge_daft_exprt_amd import vocoder_train
    with pytest.raises(ValueError, match="'f32' only"):
        voc.generator_launches(None, 'bf16x3', training=True)
    for precision in ('bf16', 'bf16x3'):
        module = voc.HiFiGANGenerator(precision=precision)
        weights = {name: (module.get_submodule(name).weight_v, module.get_submodule(name).bias) for name in module.layer_names()}
        with pytest.raises(RuntimeError, match=f"gradients exist for precision 'f32' only, got '{precision}'"):
            vocoder_train._forward_folded(module, torch.zeros(1, 80, 4), [4], weights)
