"""The 'bf16x3' precision mode without a GPU: the Python surface accepts it, the C ABI's operand-mode argument validates the value 2
before any launch, and the split-bf16 kernel instantiations are what they claim to be in the gfx950 code objects (bf16 MFMAs only,
no exact-f32 MFMA, no scratch)."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

from tests import helpers

# one ConvGemm call with 16-byte-aligned dummy pointers: validation runs before anything is dereferenced
_P = 4096


def _conv_gemm_args(mode, x_bf16=0):
    return (_P, 128, _P, None, _P, 128, 1, 16, 128, 128, 3, mode, 0, None, None, None, 0, 0, None, 0, 1.0, -1, x_bf16, 0, 0, None, None)


def test_set_precision_accepts_bf16x3():
    import ubisoft_laforge_daft_exprt_amd as pkg
    from ubisoft_laforge_daft_exprt_amd import ops
    assert 'bf16x3' in ops.PRECISIONS
    old = pkg.get_precision()
    try:
        pkg.set_precision('bf16x3')
        assert pkg.get_precision() == 'bf16x3'
    finally:
        pkg.set_precision(old)
    model = pkg.DaftExprt(helpers.golden_hparams())
    assert model.set_precision('bf16x3') is model and model.runtime.precision == 'bf16x3'
    crit = pkg.DaftExprtLoss('cpu', helpers.golden_hparams())
    assert crit.set_precision('bf16x3') is crit and crit.runtime.precision == 'bf16x3'
    assert ops.hidden_dtype('bf16x3') is torch.float32
    assert [ops._mode(p) for p in ('f32', 'bf16', 'bf16x3')] == [0, 1, 2]
    assert [ops._half(p) for p in ('f32', 'bf16', 'bf16x3')] == [0, 1, 0]     # storage: bf16x3 keeps every tensor fp32
    with pytest.raises(ValueError):
        pkg.set_precision('bf16x4')
    with pytest.raises(ValueError):
        model.set_precision('tf32')


def test_bf16x3_reads_the_f32_weight_pack():
    from ubisoft_laforge_daft_exprt_amd import ops
    pk = ops.PackedWeight(torch.zeros(8, 8, 3))
    assert ops._pack_prec('bf16x3') == 'f32' and ops._pack_prec('bf16') == 'bf16'
    img = pk._image('bf16x3')
    assert img is pk._image('f32') and img.half == 0 and list(pk._images) == ['f32']


def test_operand_mode_validation_without_gpu():
    from ubisoft_laforge_daft_exprt_amd._lib import DxError, lib
    L = lib()
    with pytest.raises(DxError, match='operand mode'):
        L.dx_conv_gemm(*_conv_gemm_args(3))
    with pytest.raises(DxError, match='operand mode'):
        L.dx_conv_gemm(*_conv_gemm_args(-1))
    with pytest.raises(DxError, match='bf16 storage'):
        L.dx_conv_gemm(*_conv_gemm_args(2, x_bf16=1))
    with pytest.raises(DxError, match='operand mode'):
        L.dx_conv_gemm_f16(*_conv_gemm_args(2))
    wg = lambda mode, dy_bf16=0: (_P, 128, _P, 128, _P, 1, 16, 128, 128, 3, None, -1, mode, dy_bf16, 0, None, None, None)
    with pytest.raises(DxError, match='operand mode'):
        L.dx_conv_wgrad(*wg(3))
    with pytest.raises(DxError, match='bf16 storage'):
        L.dx_conv_wgrad(*wg(2, dy_bf16=1))
    with pytest.raises(DxError, match='operand mode'):
        L.dx_conv_wgrad_f16(*wg(2))
    fwd = lambda mode, qkv_bf16=0: (_P, 384, _P, _P, 128, _P, 1, 16, 2, 128, 0, None, 0.0, mode, qkv_bf16, 0, None, None)
    with pytest.raises(DxError, match='operand mode'):
        L.dx_attention_fwd(*fwd(3))
    with pytest.raises(DxError, match='bf16'):
        L.dx_attention_fwd(*fwd(2, qkv_bf16=1))
    with pytest.raises(DxError, match='operand mode'):
        L.dx_attention_fwd_f16(*fwd(2))
    bwd = lambda mode: (_P, 384, _P, _P, 128, _P, _P, _P, _P, 384, 1, 16, 2, 128, 0, None, 0.0, mode, 0, 0, 0, None, None)
    with pytest.raises(DxError, match='operand mode'):
        L.dx_attention_bwd(*bwd(3))
    with pytest.raises(DxError, match='operand mode'):
        L.dx_attention_bwd_f16(*bwd(2))


# ---- disassembly guard ----------------------------------------------------------------------------------------------------
SPLIT_KERNELS = {   # source -> {mangled-name fragment: instantiations expected}
    'dx_gemm.hip': {'conv_gemm_kernelINS_9dx_split3E': 4,      # taps 1 / 3 x 64- / 128-token tiles
                    'wgrad_split_kernel': 2},                  # taps 1 / 3
    'dx_attention.hip': {'attn_fwd_split_kernel': 1, 'attn_bwd_dq_split_kernel': 1, 'attn_bwd_dkv_split_kernel': 1},
}


def _functions(asm):
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end', asm, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


@pytest.fixture(scope='module', params=sorted(SPLIT_KERNELS))
def split_asm(request):
    from ubisoft_laforge_daft_exprt_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'out.s')
        r = subprocess.run(['hipcc', *build.FLAGS, '--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage',
                            os.path.join(build.CSRC, request.param), '-o', out], capture_output=True, text=True, check=True)
        return SPLIT_KERNELS[request.param], open(out).read(), r.stderr


def test_split_instantiations_use_bf16_mfma_only(split_asm):
    kernels, asm, _ = split_asm
    funcs = _functions(asm)
    for frag, n in kernels.items():
        found = {k: v for k, v in funcs.items() if frag in k}
        assert len(found) == n, (frag, sorted(found))
        for name, body in found.items():
            assert 'v_mfma_f32_16x16x32_bf16' in body, name
            assert 'v_mfma_f32_16x16x4' not in body, name
            assert 'v_cvt_pk_bf16_f32' in body, name       # the RNE split


def test_split_instantiations_use_no_scratch(split_asm):
    kernels, _, remarks = split_asm
    usage, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r'(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)', line)
        if m and cur:
            usage.setdefault(cur, {})[m.group(1).split()[0]] = int(m.group(2))
    for frag, n in kernels.items():
        found = {k: v for k, v in usage.items() if frag in k}
        assert len(found) == n, (frag, sorted(found))
        for name, u in found.items():
            assert u['ScratchSize'] == 0, (name, u)
            assert u['Occupancy'] >= 2, (name, u)          # __launch_bounds__(256, 2): the f32 kernels' occupancy
