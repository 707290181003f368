"""Writes tests/golden/launch_plans.json: which kernel, tile width, chunk, rounds and row counts the host side of the GEMM family and of
the LayerNorm row passes picks for a shape, as the Python restatements of those rules answered before the library reported its own plan.
tests/test_launch_plans_cpu.py asks the library's ``dx_*_plan`` entry points and ``profiling``'s labels for the same rows and requires
equality, so a change that is meant to move no shape to another kernel is checked on the CPU.

The file was written ONCE, from the commit before the plan entry points, and is not regenerated from later code: the functions it reads
(``gemm_exact_helpers.conv_path`` / ``pack_dims`` / ``wgrad_path`` / ``wgrad_chunk`` / ``wgrad_batch_rounds`` / ``ff_pair_tile``,
``ln_exact_helpers.fwd_rows_per_sweep`` / ``fwd_passes`` / ``bwd_form``, ``profiling._conv_route``, the wgrad label of ``profiling.price``
and the tile arithmetic of ``ops.ff_pair_applies``) left with that change.

    python tests/golden/make_golden_launch_plans.py

Rows (every value an integer or a short name; MODES: 'bf16x3' is the split mode, which tiles as f32 does and reads the f32 pack):
  conv           [mode, B, N, Cin, Cout, taps, ldx, path, CoutP, CinP, label]       path: conv_path, label: _conv_route
  conv_label_without_2_31_guard
                 the same row layout, the rows on which _conv_route disagreed with conv_path: it never had the deep-K route's
                 ``B * N * ldx < 2^31`` guard.  The library sides with conv_path (the label of those rows is NOT what it launches).
  wgrad          [mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16, path, chunk, label]    chunk: wgrad_chunk, 32 on the f32 kernel
  wgrad_label_without_ld_rule
                 the same layout, the rows on which price()'s label disagreed with wgrad_path: it looked at Cin and Cout, never at the
                 leading dimensions, which send a 16-bit mode to the f32 kernel too.  The library sides with wgrad_path.
  wgrad_batched  [taps, [[Cin, Cout], ...], rounds]
  ff_pair        [B, N, tok, applies]      tok: ff_pair_tile (== ln_exact_helpers.ff_tile, asserted here), applies: ops.ff_pair_applies
  ln_fwd         [B, N, C, rows per sweep, passes]
  ln_bwd         [B, N, C, waves, rows per block]
  pack_dims      [Cout, Cin, half, CoutP_f, CinP_f, CinP_b, CoutP_b]
"""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(os.path.dirname(HERE)) not in sys.path:         # run as a script: the package is two directories up
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import gemm_exact_helpers as gx, ln_exact_helpers as lx  # noqa: E402
from ubisoft_laforge_daft_exprt_amd import ops, profiling  # noqa: E402

OUT = os.path.join(HERE, 'launch_plans.json')
MODES = {'f32': 0, 'bf16': 1, 'fp16': 1, 'bf16x3': 2}
TILED = {'f32': 'f32', 'bf16': 'bf16', 'fp16': 'fp16', 'bf16x3': 'f32'}       # the mode whose tiling rule a mode follows
GEOM = profiling.Geometry([])

# ---- dx_conv_gemm --------------------------------------------------------------------------------------------------------------
# (B, N, Cin, Cout, taps) of tests/test_gemm_exact_gpu.py (CONV_F32, CONV_H16, the changed-operand control) and test_gemm_exact_cpu.py
CONV_TESTS = ([(3, 129, 80, 136, 3), (5, 1, 192, 128, 1), (64, 200, 64, 1024, 3), (64, 200, 64, 1024, 1),
               (4, 37, 192, 384, 1), (3, 150, 128, 384, 1), (3, 150, 128, 1024, 3), (2, 130, 80, 136, 3), (4, 130, 288, 128, 3),
               (64, 200, 192, 1024, 1)]
              + [(13, 640, ci, co, t) for ci in (128, 80) for co in (136, 384) for t in (1, 3)]
              + [(4, 300, ci, co, t) for ci in (256, 320, 1024) for co in (128, 80) for t in (1, 3)]
              + [(70, 250, 128, 1024, 3), (1100, 130, 256, 128, 3), (1100, 130, 128, 256, 1), (2, 130, 1024, 128, 3),
                 (12, 640, 128, 384, 1)])
CONV_EDGES = ([(2, 130, ci, 128, t) for ci in (64, 68, 124, 128, 132, 192, 196, 252, 256, 260, 316, 320) for t in (1, 3)]   # CinP 128 / 256, Cin % 8, % 64
              + [(b, n, 128, 128, t) for b, n in ((1, 63 * 128), (1, 64 * 128), (1, 65 * 128), (63, 128), (64, 128), (65, 128), (32, 129), (31, 129))
                 for t in (1, 3)]                                                                                         # 63 / 64 / 65 token tiles
              + [(b, 1, 192, co, t) for b, co in ((1023, 128), (1024, 128), (1025, 128), (341, 384), (342, 384), (511, 136), (512, 136))
                 for t in (1, 3)])                                                                                        # small_below at 1023 / 1024
# (B, N, Cin, Cout, taps, ldx) around B * N * ldx = 2^31
CONV_2_31 = [(2048, 1024, 1024, 128, 3, 1024), (2047, 1024, 1024, 128, 3, 1024), (2048, 1024, 256, 128, 1, 1024), (2048, 1024, 256, 128, 1, 1020),
             (4096, 1024, 512, 128, 1, 512), (4096, 1024, 512, 128, 1, 516)]


def conv_rows():
    shapes = [s + (s[2],) for s in CONV_TESTS + CONV_EDGES] + [s + (s[2] + 64,) for s in CONV_TESTS] + [s + (s[2] + 4,) for s in CONV_EDGES[:24]]
    shapes += CONV_2_31
    rows, odd = [], []
    for mode, code in MODES.items():
        for B, N, Cin, Cout, taps, ldx in shapes:
            path = gx.conv_path(TILED[mode], B, N, Cin, Cout, taps, ldx=ldx)
            dims = gx.pack_dims(Cout, Cin, code == 1)
            label = profiling._conv_route(dict(bf16=code, B=B, N=N, Cin=Cin, Cout=Cout, taps=taps, ldx=ldx))
            want = {'dk': f'conv_dk_kernel<{taps}>', 'ws': f'conv_ws_kernel<{taps}>', 'h16_64': 'conv_gemm_kernel<bf16>', 'h16_128': 'conv_gemm_kernel<bf16>',
                    'f32_64': 'conv_gemm_kernel<f32>', 'f32_128': 'conv_gemm_kernel<f32>'}[path]
            if code == 2:
                want = 'conv_gemm_kernel<bf16x3>'
            row = [mode, B, N, Cin, Cout, taps, ldx, path, dims[0], dims[1], label]
            if label == want:
                rows.append(row)
            else:
                assert B * N * ldx >= 2 ** 31 and label.startswith('conv_dk'), row      # the one known disagreement
                odd.append(row)
    return rows, odd


# ---- dx_conv_wgrad -------------------------------------------------------------------------------------------------------------
WGRAD_TESTS = ([(3, 65, 80, 136, 1), (3, 65, 80, 136, 3), (3, 130, 128, 384, 1), (3, 130, 128, 384, 3), (2, 90, 256, 136, 3), (2, 130, 1024, 512, 1),
                (2, 130, 1024, 512, 3), (5, 17, 192, 4, 1), (520, 20, 128, 136, 1), (2, 130, 192, 4, 1)]
               + [(2, n, 128, 136, t) for t in (3, 1) for n in (63, 64, 65, 127, 128, 129)] + [(2, n, 1024, 512, 3) for n in (65, 127)])
WGRAD_EDGES = ([(2, 130, ci, co, t) for ci, co in ((128, 3968), (128, 4096), (384, 1280), (384, 1408), (512, 896), (512, 1024), (576, 896), (192, 2816),
                                                   (896, 512), (896, 640), (1024, 384), (1024, 512))
                for t in (1, 3)]                                                                    # the wide rule either side of 64 tile products
               + [(2, 130, ci, co, 1) for ci, co in ((4, 128), (12, 128), (68, 136), (132, 128), (128, 4), (128, 132), (128, 12), (260, 260))])   # % 8


def wgrad_rows():
    shapes = [s + (s[2], s[3]) for s in WGRAD_TESTS + WGRAD_EDGES]
    shapes += [s + (s[2] + 4, s[3]) for s in WGRAD_TESTS[:8] + WGRAD_EDGES[:6]] + [s + (s[2], s[3] + 4) for s in WGRAD_TESTS[:8] + WGRAD_EDGES[:6]]
    shapes += [s + (s[2] + 8, s[3] + 16) for s in WGRAD_TESTS[:8]]
    rows, odd = [], []
    for mode, code in MODES.items():
        for B, N, Cin, Cout, taps, ldx, ldy in shapes:
            path = gx.wgrad_path(TILED[mode], Cin, Cout, ldx=ldx, ldy=ldy)
            for dy16, x16 in ([(a, b) for a in (0, 1) for b in (0, 1)] if path != 'f32' else [(0, 0)]):
                chunk = gx.wgrad_chunk(taps, bool(dy16), bool(x16)) if path != 'f32' else 32
                label = profiling.price('dx_conv_wgrad', dict(B=B, N=N, Cin=Cin, Cout=Cout, taps=taps, bf16=code, dy_bf16=dy16, x_bf16=x16,
                                                              ldx=ldx, ldy=ldy, lens=0), GEOM)[0]
                want = {'f32': f'wgrad_kernel<{taps}>', 'narrow': f'wgrad_bf16_kernel<{taps}>', 'wide': f'wgrad_bf16_kernel<{taps},wide>'}[path]
                if code == 2:
                    want = f'wgrad_split_kernel<{taps},bf16x3>'
                row = [mode, B, N, Cin, Cout, taps, ldx, ldy, dy16, x16, path, chunk, label]
                if label == want:
                    rows.append(row)
                else:
                    assert code == 1 and path == 'f32' and (ldx % 8 or ldy % 8) and Cin % 8 == 0 and Cout % 8 == 0, row
                    odd.append(row)
    return rows, odd


def wgrad_batched_rows():
    geo = [(128, 128, 2 * 100), (128, 384, 3 * 77), (256, 128, 2 * 130), (128, 1024, 1 * 65)]         # test_wgrad_batched_launch: (Cin, Cout, B * N)
    order = sorted((geo[i % 4] for i in range(34)), key=lambda j: -j[2])
    sets = [[list(j[:2]) for j in order[k:k + ops.WGRAD_BATCH[taps]]] for taps in (1, 3) for k in range(0, 34, ops.WGRAD_BATCH[taps])]
    sets += [[[128, 128 * n]] for n in (1, 31, 32, 95, 96, 97, 160)] + [[[128, 128]] * n for n in (2, 31, 32)] + [[[1024, 1024]] * n for n in (1, 2, 24)]
    sets += [[[128, 1024]] * 24, [[128, 136], [256, 8], [384, 264]]]
    return [[taps, s, gx.wgrad_batch_rounds([tuple(j) for j in s])] for taps in (1, 3) for s in sets]


# ---- the fused feed-forward pair -----------------------------------------------------------------------------------------------
def ff_rows():
    pack = types.SimpleNamespace(taps=3, cin=128, cout=128)
    shapes = [(4, 127), (32, 379), (23, 379), (5, 300), (35, 300), (48, 120), (1, 95 * 126), (1, 96 * 126), (1, 96 * 126 + 1), (1, 63 * 62), (1, 64 * 62),
              (1, 63 * 62 + 1)]
    shapes += [(b, n) for b in (1, 2, 31, 32, 33, 47, 48, 63, 64, 65, 95, 96, 97) for n in (1, 62, 63, 124, 125, 126, 127, 252, 253)]
    rows = []
    for B, N in shapes:
        tok = gx.ff_pair_tile(B, N)
        assert tok == lx.ff_tile(B, N)
        x = torch.empty(B, N, 128, dtype=torch.bfloat16, device='meta')
        rows.append([B, N, tok, int(ops.ff_pair_applies(x, pack, pack, 'bf16'))])
    return rows


# ---- dx_ln_fwd / dx_ln_bwd -----------------------------------------------------------------------------------------------------
LN_SHAPES = [(3, 70), (64, 257), (129, 255), (1, 16383), (1, 16384), (1, 16385), (128, 128), (127, 129), (5, 300), (35, 300), (3, 9), (1, 1), (1, 3),
             (1, 4), (1, 5), (1, 16), (1, 17), (1, 32764), (1, 32765), (1, 32767), (1, 32768), (1, 32769), (1, 40000), (8, 8192), (1, 65536), (1, 65537)]


def ln_rows():
    fwd = [[B, N, C, lx.fwd_rows_per_sweep(B * N, C), lx.fwd_passes(B * N, C)] for C in (128, 1024) for B, N in LN_SHAPES]
    bwd = [[B, N, C, *lx.bwd_form(B, N, C)] for C in (128, 1024) for B, N in LN_SHAPES]
    return fwd, bwd


def pack_rows():
    shapes = [(3, 80), (3, 192), (136, 80), (384, 128), (128, 1024), (1024, 128), (80, 256), (128, 128), (136, 192), (4, 192), (256, 80), (384, 320),
              (80, 288), (128, 64), (128, 288), (1, 1), (129, 33), (127, 31)]
    return [[co, ci, half, *gx.pack_dims(co, ci, half)] for half in (0, 1) for co, ci in shapes]


def record():
    conv, conv_odd = conv_rows()
    wgrad, wgrad_odd = wgrad_rows()
    fwd, bwd = ln_rows()
    return {'conv': conv, 'conv_label_without_2_31_guard': conv_odd, 'wgrad': wgrad, 'wgrad_label_without_ld_rule': wgrad_odd,
            'wgrad_batched': wgrad_batched_rows(), 'ff_pair': ff_rows(), 'ln_fwd': fwd, 'ln_bwd': bwd, 'pack_dims': pack_rows()}


def dumps(recorded):
    """one row per line, so that a mismatch reads as a diff"""
    lines = ['{']
    for i, (key, rows) in enumerate(recorded.items()):
        lines.append(f' {json.dumps(key)}: [')
        lines += ['  ' + json.dumps(r, separators=(',', ':')) + (',' if k + 1 < len(rows) else '') for k, r in enumerate(rows)]
        lines.append(' ]' + (',' if i + 1 < len(recorded) else ''))
    lines.append('}')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    recorded = record()
    with open(OUT, 'w') as f:
        f.write(dumps(recorded))
    print(', '.join(f'{key} {len(rows)}' for key, rows in recorded.items()))
