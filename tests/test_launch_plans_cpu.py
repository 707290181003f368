"""CPU checks of the library's launch plans (``dx_conv_gemm_plan``, ``dx_conv_wgrad_plan``, ``dx_conv_wgrad_batched_plan``, ``dx_ff_pair_plan``,
``dx_ln_plan``; include/daft_exprt_hip.h) and of the labels ``profiling`` makes from them, row by row against what the Python restatements of
the same rules answered before the dispatchers reported their own plan (tests/golden/make_golden_launch_plans.py)."""
import json
import os
import types

import pytest
import torch

from tests import gemm_exact_helpers as gx, ln_exact_helpers as lx
from ubisoft_laforge_daft_exprt_amd import _lib, ops, profiling

GEOM = profiling.Geometry([])


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_plans.json')) as f:
        return json.load(f)


def conv_label(mode, B, N, Cin, Cout, taps, ldx):
    a = dict(B=B, N=N, Cin=Cin, Cout=Cout, taps=taps, bf16=gx.OPERAND_MODE[mode], ldx=ldx, x_bf16=0, y_bf16=0, aux_bf16=0, accumulate=0)
    return profiling.price('dx_conv_gemm_f16' if mode == 'fp16' else 'dx_conv_gemm', a, GEOM)[0]


def wgrad_label(mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16):
    a = dict(B=B, N=N, Cin=Cin, Cout=Cout, taps=taps, bf16=gx.OPERAND_MODE[mode], ldx=ldx, ldy=ldy, dy_bf16=dy16, x_bf16=x16)
    return profiling.price('dx_conv_wgrad', a, GEOM)[0]


def as_restated(path, mode):
    """the split mode tiles as f32 does: the restatement had no name of its own for it"""
    return path.replace('split', 'f32') if mode == 'bf16x3' else path


def test_the_file_holds_every_family_and_threshold(recorded):
    assert {k: len(v) for k, v in recorded.items()} == {'conv': 608, 'conv_label_without_2_31_guard': 8, 'wgrad': 634, 'wgrad_label_without_ld_rule': 52,
                                                       'wgrad_batched': 44, 'ff_pair': 129, 'ln_fwd': 52, 'ln_bwd': 52, 'pack_dims': 36}
    assert {r[7] for r in recorded['conv']} == {'f32_64', 'f32_128', 'h16_64', 'h16_128', 'ws', 'dk'}
    assert {r[10] for r in recorded['wgrad']} == {'f32', 'narrow', 'wide'} and {r[11] for r in recorded['wgrad']} == {32, 64, 128}
    assert {(r[2], r[3]) for r in recorded['ff_pair']} == {(62, 0), (62, 1), (126, 1)}
    assert {tuple(r[3:]) for r in recorded['ln_bwd']} == {(4, 64), (16, 192), (4, 32)} and {r[4] for r in recorded['ln_fwd']} == {1, 2, 3}


def test_conv_plans_and_labels_reproduce_the_record(recorded):
    for mode, B, N, Cin, Cout, taps, ldx, path, coutp, cinp, label in recorded['conv']:
        p = gx.conv_plan(mode, B, N, Cin, Cout, taps, ldx)
        row = (mode, B, N, Cin, Cout, taps, ldx)
        assert (as_restated(gx.path(p), mode), p.coutp, p.cinp) == (path, coutp, cinp), row
        assert conv_label(*row) == label, row
        assert p.grid_x > 0 and p.grid_y == coutp // 128 and p.threads == (256 if p.kernel.startswith('conv_gemm') else 512), row


def test_at_two_to_the_31_the_library_sides_with_the_guarded_restatement(recorded):
    """the one known disagreement of the two restatements: the label function had no ``B * N * ldx < 2^31`` guard on the deep-K route"""
    for mode, B, N, Cin, Cout, taps, ldx, path, coutp, cinp, label in recorded['conv_label_without_2_31_guard']:
        assert B * N * ldx >= 2 ** 31 and label == f'conv_dk_kernel<{taps}>' and path == 'h16_128'
        assert gx.path(gx.conv_plan(mode, B, N, Cin, Cout, taps, ldx)) == path
        assert conv_label(mode, B, N, Cin, Cout, taps, ldx) == 'conv_gemm_kernel<bf16>'


def test_wgrad_plans_and_labels_reproduce_the_record(recorded):
    for mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16, path, chunk, label in recorded['wgrad']:
        p = gx.wgrad_plan(mode, B, N, Cin, Cout, taps, dy16, x16, ldx, ldy)
        row = (mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16)
        assert (as_restated(gx.path(p), mode), p.chunk) == (path, chunk), row
        assert wgrad_label(*row) == label, row
        assert 1 <= p.split == p.grid_z <= B * -(-N // chunk) and p.threads == {'f32': 256, 'narrow': 256, 'wide': 512}[path], row


def test_a_leading_dimension_off_8_sends_the_16_bit_modes_to_the_f32_kernel(recorded):
    """a second disagreement, found while recording: the label function looked at Cin and Cout only.  The library sides with the path."""
    for mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16, path, chunk, label in recorded['wgrad_label_without_ld_rule']:
        assert (ldx % 8 or ldy % 8) and path == 'f32' and label.startswith('wgrad_bf16_kernel')
        p = gx.wgrad_plan(mode, B, N, Cin, Cout, taps, dy16, x16, ldx, ldy)
        assert (gx.path(p), p.chunk) == (path, chunk)
        assert wgrad_label(mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16) == f'wgrad_kernel<{taps}>'


def test_batched_wgrad_plans_reproduce_the_record(recorded):
    for taps, shapes, rounds in recorded['wgrad_batched']:
        for mode in ('bf16', 'fp16'):
            p = gx.wgrad_batched_plan(mode, taps, [(2, 130, ci, co) for ci, co in shapes])
            assert p.rounds == rounds and p.kernel == 'wgrad_h16_wide' and (p.grid_y, p.threads) == (len(shapes), 512), (taps, shapes)
    with pytest.raises(_lib.DxError, match='multiple of 128'):
        gx.wgrad_batched_plan('bf16', 1, [(2, 130, 64, 128)])


def test_ff_pair_plans_and_the_fused_rule_reproduce_the_record(recorded):
    pack = types.SimpleNamespace(taps=3, cin=128, cout=128)
    for B, N, tok, applies in recorded['ff_pair']:
        p = gx.ff_pair_plan(B, N)
        assert p == gx.ff_pair_plan(B, N, 'fp16') and (p.tok, p.grid_x, p.threads) == (tok, B * -(-N // tok), 512), (B, N)
        assert lx.ff_pair_tok(B, N) == tok
        x = torch.empty(B, N, 128, dtype=torch.bfloat16, device='meta')
        assert ops.ff_pair_applies(x, pack, pack, 'bf16') == bool(applies), (B, N)


def test_layernorm_plans_reproduce_the_record(recorded):
    for B, N, C, sweep, passes in recorded['ln_fwd']:
        p = lx.ln_plan(B, N, C)
        assert (p.kernel, p.sweep, p.passes) == ('ln_fwd', sweep, passes) and p.grid_x * p.tok == sweep, (B, N, C)
    for B, N, C, waves, rpb in recorded['ln_bwd']:
        p = lx.ln_plan(B, N, C, backward=True)
        assert (p.kernel, p.threads, p.tok) == ('ln_bwd', 64 * waves, rpb) and (p.grid_x, p.grid_y) == (-(-N // rpb), B), (B, N, C)
        assert lx.bwd_waves_rows(B, N, C) == (waves, rpb)


def test_pack_dims_reproduce_the_record(recorded):
    import ctypes
    for cout, cin, half, *dims in recorded['pack_dims']:
        out = (ctypes.c_int * 4)()
        _lib.lib().dx_pack_dims(cout, cin, half, ctypes.addressof(out))
        assert list(out) == dims
        fwd, bwd = (gx.conv_plan('bf16' if half else 'f32', 1, 1, ci, co, 1) for ci, co in ((cin, cout), (cout, cin)))
        assert [fwd.coutp, fwd.cinp, bwd.coutp, bwd.cinp] == dims


def test_plans_validate_and_the_fp16_build_rejects_the_split_mode():
    assert gx.path(gx.conv_plan('bf16x3', 3, 129, 80, 136, 3)) == 'split_64' and gx.path(gx.wgrad_plan('bf16x3', 3, 65, 80, 136, 1)) == 'split'
    for entry, args in (('dx_conv_gemm_plan_f16', (3, 129, 80, 136, 3, 2, 80)), ('dx_conv_wgrad_plan_f16', (3, 65, 80, 136, 1, 2, 80, 136, 0, 0))):
        with pytest.raises(_lib.DxError, match='operand mode'):
            _lib.plan(entry, *args)
    with pytest.raises(_lib.DxError, match='C must be 128 or 1024'):
        lx.ln_plan(3, 70, 256)
    with pytest.raises(_lib.DxError, match='bad dims'):
        gx.conv_plan('f32', 0, 129, 80, 136, 3)
    Plan, kernels = _lib._plan_layout()
    assert Plan._fields[:6] == ('kernel', 'tok', 'grid_x', 'grid_y', 'grid_z', 'threads') and len(set(kernels)) == len(kernels) == 12
