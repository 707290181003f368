"""CPU checks of the HiFi-GAN vocoder's host side: state-dict layout, weight-norm folding, checkpoint forms, argument validation,
the plain-torch restatement against the reference golden, and the generated ISA of csrc/dx_vocoder.hip."""
import copy
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from torch.nn.utils import remove_weight_norm, weight_norm

from tests import vocoder_helpers as vh
from tests import vocoder_torch
from ubisoft_laforge_daft_exprt_amd import vocoder as voc

PKG = os.path.dirname(os.path.abspath(voc.__file__))


def test_state_dict_keys_and_shapes_match_reference_manifest():
    gen = voc.HiFiGANGenerator(voc.DEFAULT_CONFIG)
    sd = gen.state_dict()
    man = vh.manifest()['keys']
    assert voc.DEFAULT_CONFIG == vh.manifest()['config']           # the V1 restatement is the configuration the reference ships
    assert len(sd) == len(man) == 234
    assert sorted(sd) == sorted(man)
    for k, shape in man.items():
        assert list(sd[k].shape) == shape, k
    assert list(sd['ups.0.weight_g'].shape) == [512, 1, 1]          # per INPUT channel of the (512, 256, 16) ConvTranspose1d weight
    gen.load_state_dict(vh.state_dict(), strict=True)


def test_weight_norm_folding_equals_torch_remove_weight_norm():
    sd = vh.state_dict()
    gen = voc.HiFiGANGenerator()
    gen.load_state_dict(sd, strict=True)
    folded = gen.folded()
    for name in gen.layer_names():
        v, g = sd[name + '.weight_v'], sd[name + '.weight_g']
        if name.startswith('ups.'):
            m = torch.nn.ConvTranspose1d(v.shape[0], v.shape[1], v.shape[2])
        else:
            m = torch.nn.Conv1d(v.shape[1], v.shape[0], v.shape[2])
        m = weight_norm(m)
        m.weight_v.data.copy_(v)
        m.weight_g.data.copy_(g)
        remove_weight_norm(m)
        assert torch.equal(folded[name][0], m.weight.data), name
        assert torch.equal(folded[name][1], sd[name + '.bias']), name


def test_every_checkpoint_form_loads_the_same_folded_weights(tmp_path):
    sd = vh.state_dict()
    plain_vocoder = voc.HiFiGanVocoder(sd, device='cpu')
    plain = plain_vocoder.weights
    assert all(torch.equal(v, sd[k]) for k, v in plain_vocoder.generator.state_dict().items())
    gen = voc.HiFiGANGenerator()
    gen.load_state_dict(sd)
    folded_sd = {}
    for name, (w, b) in gen.folded().items():
        folded_sd[name + '.weight'], folded_sd[name + '.bias'] = w, b
    forms = [{'generator': sd}, {'state_dict': sd}, sd, {'generator': folded_sd}, folded_sd]
    for i, form in enumerate(forms):
        path = os.path.join(str(tmp_path), f'g{i}.pth')
        torch.save(form, path)
        loaded = voc.load_hifigan_vocoder(path, device='cpu')
        assert (loaded.generator is None) == (form is folded_sd or form.get('generator') is folded_sd)     # folded: no weight-normed copy
        got = loaded.weights
        assert sorted(got) == sorted(plain)
        for k in plain:
            assert torch.equal(got[k][0], plain[k][0]) and torch.equal(got[k][1], plain[k][1]), (i, k)
    with pytest.raises(KeyError, match='conv_post'):
        voc.HiFiGanVocoder({k: v for k, v in sd.items() if not k.startswith('conv_post')}, device='cpu')


def test_no_download_path():
    with pytest.raises(ValueError, match='checkpoint_path'):
        voc.HiFiGanVocoder(None)
    with pytest.raises(ValueError, match='checkpoint_path'):
        voc.load_hifigan_vocoder()
    src = open(voc.__file__).read()
    assert not re.search(r'^\s*(import|from)\s+(urllib|huggingface_hub|requests|http)\b', src, flags=re.M)


def test_infer_rejects_a_batch():
    v = voc.HiFiGanVocoder(vh.state_dict(), device='cpu')
    with pytest.raises(ValueError, match='batch'):
        v.infer(np.zeros((2, 80, 5), dtype=np.float32))


def test_voc_entry_points_reject_aliasing_and_misalignment_before_any_launch():
    from ubisoft_laforge_daft_exprt_amd._lib import lib, DxError
    with pytest.raises(DxError, match='alias'):
        lib().dx_voc_conv(4096, 64 * 8, 64, 1, 1, None, 4096, 64 * 8, None, 1, 1, 1, 8, 64, 64, 3, 1, 1, 1, 0, 0, None)
    with pytest.raises(DxError, match='aligned'):
        lib().dx_voc_conv(4100, 64 * 8, 64, 1, 1, None, 8192, 64 * 8, None, 1, 1, 1, 8, 64, 64, 3, 1, 1, 1, 0, 0, None)
    with pytest.raises(DxError, match='aligned'):
        lib().dx_voc_pair(4100, 64 * 8, 1, 1, 1, 1, 8192, 1, 1, 1, 8, 64, 3, 1, 0, 0, None)
    with pytest.raises(DxError, match='aligned'):
        lib().dx_voc_post(4100, 32 * 8, 1, 1, 8192, 8, 1, 1, 1, 8, 8, None)


def test_precision_and_config_validation():
    sd = vh.state_dict()
    with pytest.raises(ValueError, match='precision'):
        voc.HiFiGanVocoder(sd, device='cpu', precision='fp16')
    for key, value in (('resblock', '2'), ('upsample_rates', [8, 8, 4]), ('upsample_initial_channel', 256)):
        cfg = copy.deepcopy(voc.DEFAULT_CONFIG)
        cfg[key] = value
        with pytest.raises(NotImplementedError):
            voc.HiFiGANGenerator(cfg)
        with pytest.raises(NotImplementedError):
            voc.HiFiGanVocoder(sd, config=cfg, device='cpu')
    assert voc.HiFiGanVocoder(sd, device='cpu', precision='bf16').precision == 'bf16'
    with pytest.raises(RuntimeError, match='GPU'):
        voc.HiFiGanVocoder(sd, device='cpu').infer(np.zeros((80, 3), dtype=np.float32))


def test_torch_restatement_matches_reference_golden():
    lengths, mels, wavs = vh.golden()
    weights = voc.fold_state_dict(vh.state_dict(), voc.HiFiGANGenerator().layer_names())
    for n, mel, ref in zip(lengths, mels, wavs):
        with torch.no_grad():
            got = vocoder_torch.generator(torch.from_numpy(mel)[None], weights)[0].numpy()
        assert got.shape == (256 * n,)
        assert np.abs(got - ref).max() <= 1e-5, n


def test_vocoder_isa_has_no_packed_f32_with_swapped_op_sel():
    if shutil.which('hipcc') is None:
        pytest.skip('hipcc not on PATH')
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'dx_vocoder.s')
        subprocess.run(['hipcc', '-O3', '--offload-arch=gfx950', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(PKG, 'csrc', 'dx_vocoder.hip')], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    bad = [ln.strip() for ln in text.splitlines() if re.search(r'v_pk_(fma|mul|add)_f32', ln) and re.search(r'\bop_sel:\[[^\]]*1', ln)]
    assert not bad, bad[:4]
    assert 'voc_pair_kernel' in text and 'voc_conv_kernel' in text
