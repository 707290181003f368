"""Per-kernel roofline accounting for bench.py and tools/ (measurement support: nothing here computes anything on the path).

``_lib.set_timer(list)`` makes every C-ABI launch record (entry point, its C arguments by name, start event, stop event) on the
stream the kernels run on.  ``price()`` turns one record into ALGORITHMIC work -- FLOPs for the MFMA-bound kernels, HBM bytes for
the memory-bound ones -- following SURVEY.md §8(d): valid tokens only (padding the kernels compute or skip is not credited),
multiply-add = 2, every tensor the operation must read or write counted once at its storage width.  ``summarize()`` groups the
records of a step by kernel and divides by the measured durations.

Peaks: /opt/skills/guides/MI355X_MICROARCH.md §Chip-level parameters (HBM3E 8.0 TB/s spec; dense MFMA 2.5 PFLOP/s bf16, 157.3
TFLOP/s f32-input).
"""
from __future__ import annotations

from collections import OrderedDict

# 'bf16x3': an fp32-EQUIVALENT peak -- the bf16 rate over the three split-bf16 MFMAs each fp32 product costs (FLOPs are counted once)
PEAK_TFLOPS = {'f32': 157.3, 'bf16': 2500.0, 'bf16x3': 2500.0 / 3}
PEAK_HBM_GBS = 8000.0


class Geometry:
    """valid rows and sum of squared lengths per padded axis length N of the batch (frames and symbols)."""

    def __init__(self, axes):
        """``axes``: iterable of 1-D integer sequences of per-utterance lengths (one per axis)."""
        self.by_n = {}
        for lens in axes:
            lens = [int(v) for v in lens]
            self.by_n[(len(lens), max(lens))] = (sum(lens), sum(v * v for v in lens))

    def rows(self, B, N, lens_ptr=True):
        if not lens_ptr:
            return B * N
        return self.by_n.get((B, N), (B * N, B * N * N))[0]

    def pairs(self, B, N):
        return self.by_n.get((B, N), (B * N, B * N * N))[1]


# kernel id of a launch plan (include/daft_exprt_hip.h DX_K_*, as _lib.plan names it) -> the label's text, ``{}`` = taps
_LABELS = {'conv_gemm_f32': 'conv_gemm_kernel<f32>', 'conv_gemm_h16': 'conv_gemm_kernel<bf16>', 'conv_gemm_split': 'conv_gemm_kernel<bf16x3>',
           'conv_dk': 'conv_dk_kernel<{}>', 'conv_ws': 'conv_ws_kernel<{}>', 'wgrad_f32': 'wgrad_kernel<{}>', 'wgrad_split': 'wgrad_split_kernel<{},bf16x3>',
           'wgrad_h16': 'wgrad_bf16_kernel<{}>', 'wgrad_h16_wide': 'wgrad_bf16_kernel<{},wide>'}


def _label(entry, a, *names):
    """The label of the kernel the library's dispatcher launches for the recorded arguments ``a``: its own plan, asked with ``names``
    (a record without a leading dimension is a dense tensor: ldx = Cin, ldy = Cout)."""
    from ._lib import plan
    a = dict({'ldx': a['Cin'], 'ldy': a['Cout']}, **a)
    return _LABELS[plan(entry, *(int(a[k]) for k in names)).kernel].format(a['taps'])


def price(name, a, geom: Geometry):
    """-> (kernel label, bound, algorithmic FLOPs, algorithmic HBM bytes); bytes / FLOPs may be None when not modelled."""
    g = a.get
    has = lambda k: bool(g(k))
    if name.endswith('_f16'):                            # the fp16 twins (include/daft_exprt_hip.h): same kernels, same work
        name = name[:-4]
    if name == 'dx_conv_gemm':
        rows = geom.rows(a['B'], a['N'], has('lens'))
        xb, yb, ab = (2 if a['x_bf16'] else 4), (2 if a['y_bf16'] else 4), (2 if a['aux_bf16'] else 4)
        wb = 2 if a['bf16'] == 1 else 4
        byt = rows * (a['Cin'] * xb + a['Cout'] * yb * (2 if a['accumulate'] else 1) + (a['Cout'] * ab if has('relu_aux') else 0)) \
            + a['taps'] * a['Cin'] * a['Cout'] * wb
        return _label('dx_conv_gemm_plan', a, 'B', 'N', 'Cin', 'Cout', 'taps', 'bf16', 'ldx'), 'mfma', 2.0 * a['taps'] * a['Cin'] * a['Cout'] * rows, byt
    if name == 'dx_ff_pair':
        rows = geom.rows(a['B'], a['N'], has('lens'))
        F = a['F']
        byt = rows * (128 * 2 + F * 2 + 128 * 4 * (2 if a['accumulate'] else 1) + (F * 2 if has('aux') else 0)) + 2 * 3 * 128 * F * 2
        return 'ff_pair_kernel<bwd>' if has('aux') else 'ff_pair_kernel<fwd>', 'mfma', 2.0 * 2 * 3 * 128 * F * rows, byt
    if name == 'dx_ff_pair_ln':                          # the forward pair + the LayerNorm epilogue: residual read, z and y written
        rows = geom.rows(a['B'], a['N'], has('lens'))
        F = a['F']
        byt = rows * (128 * 2 + F * 2 + 128 * 4 * 3 + 8) + 2 * 3 * 128 * F * 2
        return 'ff_pair_kernel<fwd>', 'mfma', 2.0 * 2 * 3 * 128 * F * rows, byt
    if name == 'dx_ff_pair_ln_qkv':                      # ... + the next block's in-projection (128 -> 384) on the normalised tile: 16-bit qkv written
        rows = geom.rows(a['B'], a['N'], has('lens'))
        F = a['F']
        byt = rows * (128 * 2 + F * 2 + 128 * 4 * 3 + 8 + 384 * 2) + 2 * 3 * 128 * F * 2 + 384 * 128 * 2
        return 'ff_pair_kernel<fwd>', 'mfma', (2.0 * 2 * 3 * 128 * F + 2.0 * 128 * 384) * rows, byt
    if name == 'dx_ff_pair_lnbwd':                       # the input-gradient pair + the LayerNorm-backward epilogue: z read, dz and the 16-bit copy written
        rows = geom.rows(a['B'], a['N'], has('lens'))
        F = a['F']
        byt = rows * (128 * 2 + 2 * F * 2 + 128 * 4 * 3 + 128 * 2 + 8) + 2 * 3 * 128 * F * 2
        return 'ff_pair_kernel<bwd>', 'mfma', 2.0 * 2 * 3 * 128 * F * rows, byt
    if name == 'dx_ff_block_bwd':                        # LN2-backward prologue + input-gradient pair + LN1-backward epilogue
        rows = geom.rows(a['B'], a['N'], has('lens'))
        F = a['F']
        byt = rows * (2 * 128 * 4 + 2 * 128 * 4 + 2 * 128 * 2 + 2 * F * 2 + 128 * 4 + 16) + 2 * 3 * 128 * F * 2   # dY2, z2, z1 read; dz2 + dz1 written; two 16-bit copies; aux + H
        return 'ff_pair_kernel<bwd>', 'mfma', 2.0 * 2 * 3 * 128 * F * rows, byt
    if name == 'dx_conv_wgrad':
        rows = geom.rows(a['B'], a['N'], has('lens'))
        byt = rows * (a['Cout'] * (2 if a['dy_bf16'] else 4) + a['Cin'] * (2 if a['x_bf16'] else 4)) + a['taps'] * a['Cin'] * a['Cout'] * 4
        label = _label('dx_conv_wgrad_plan', a, 'B', 'N', 'Cin', 'Cout', 'taps', 'bf16', 'ldx', 'ldy', 'dy_bf16', 'x_bf16')
        return label, 'mfma', 2.0 * a['taps'] * a['Cin'] * a['Cout'] * rows, byt
    if name == 'dx_conv_wgrad_batched':
        from . import ops
        jobs = ops.WGRAD_BATCH_LOG.get(a['jobs'], (None, []))[1]       # the descriptors of this launch (kept while a timer is installed)
        flops = byt = 0
        for (_dy, _x, _g, _db, lens, _ldy, _ldx, B, N, Cin, Cout, *_rest) in jobs:
            rows = geom.rows(B, N, lens is not None)
            flops += 2.0 * a['taps'] * Cin * Cout * rows
            byt += rows * (Cout * (2 if a['dy_bf16'] else 4) + Cin * (2 if a['x_bf16'] else 4)) + a['taps'] * Cin * Cout * 4
        return f"wgrad_bf16_kernel<{a['taps']},wide>", 'mfma', (flops or None), (byt or None)      # batched launches use the wide tile
    if name in ('dx_attention_fwd', 'dx_attention_bwd'):
        rows, pairs = geom.rows(a['B'], a['N']), geom.pairs(a['B'], a['N'])
        D, H = a['D'], a['H']
        qb = 2 if a['qkv_bf16'] else 4
        sfx = ' <bf16x3>' if a['bf16'] == 2 else ''         # split-bf16 kernels (priced at the fp32-equivalent peak)
        if name == 'dx_attention_fwd':                       # S = QK^T and O = PV: 2 products of 2 N^2 hd per head
            return 'attn_fwd' + sfx, 'mfma', 4.0 * pairs * D, rows * (3 * D * qb + D * 4 + H * 4)
        gb = 2 if a['dqkv_bf16'] else 4                      # dQ kernel: S, dP, dQ; dK/dV kernel: S, dP, dV, dK: 7 products
        return 'attn_bwd (dq + dkv)' + sfx, 'mfma', 14.0 * pairs * D, rows * (2 * 3 * D * qb + 2 * D * 4 + 3 * D * gb + 2 * H * 4)
    if name in ('dx_pitch_chain_fwd', 'dx_pitch_chain_bwd'):      # the frozen predictor: 3 taps x (M x 256 + 2 x 256 x 256) MACs per token + the one-channel layer
        rows = geom.rows(a['B'], a['T'], True)
        flops = 2.0 * 3 * (a['M'] * 256 + 2 * 256 * 256 + 256) * rows
        byt = rows * (a['M'] * 4 + 4 + 96 + (a['M'] * 8 if name.endswith('bwd') else 0))       # mel / pp (dpp) / sign bits; backward: dmel read + written
        return ('pitch_chain<fwd>' if name.endswith('fwd') else 'pitch_chain<bwd>'), 'mfma', flops, byt
    if name == 'dx_attention_proj_ln_fwd':               # attn_fwd + proj_ln_fwd in one launch: both products, the 128 x 128 projection, the row pass's bytes
        rows, pairs = geom.rows(a['B'], a['N']), geom.pairs(a['B'], a['N'])
        D, H = a['D'], a['H']
        byt = rows * (3 * D * 2 + D * 2 + H * 4) + rows * (128 * (4 + 4 + (4 if has('res') else 0) + (2 if has('y_bf16_copy') else 0)) + 8) + 128 * 128 * 2
        return 'attn_fwd+proj_ln', 'mfma', 4.0 * pairs * D + 2.0 * rows * 128 * 128, byt
    if name == 'dx_ln_fwd':
        rows = geom.rows(a['B'], a['N'], has('lens'))
        C, ab = a['C'], (2 if a['io_bf16'] else 4)
        byt = rows * (C * (2 * ab + 4 + (4 if has('res') else 0) + (2 if has('y_bf16_copy') else 0)) + 8)
        return f'ln_fwd_kernel<{C}>', 'hbm', None, byt
    if name == 'dx_proj_ln_fwd':                         # X (16-bit) read; z, y written, residual read (fp32); 16-bit copy of y; the 32 KB weight pack
        rows = geom.rows(a['B'], a['N'], has('lens'))
        byt = rows * (128 * (2 + 4 + 4 + (4 if has('res') else 0) + (2 if has('y_bf16_copy') else 0)) + 8) + 128 * 128 * 2
        return 'proj_ln_fwd', 'hbm', None, byt
    if name == 'dx_ln_bwd':
        rows = geom.rows(a['B'], a['N'], has('lens'))
        C, zb = a['C'], (2 if a['io_bf16'] else 4)
        byt = rows * (C * (3 * zb + (4 if has('da') else 0) + (2 if has('dg_bf16_copy') else 0)) + 8)   # dy, z read; dz (+ da, bf16 copy) written
        return f'ln_bwd_kernel<{C}>', 'hbm', None, byt
    if name == 'dx_upsample_fwd':
        B, L, T, D = a['B'], a['L'], a['T'], a['D']
        return 'upsample_fwd', 'hbm', None, B * L * D * 4 + 3 * B * L * 4 + B * T * D * 4 + B * L * T * 4
    if name == 'dx_upsample_bwd':
        B, L, T, D = a['B'], a['L'], a['T'], a['D']
        return 'upsample_bwd (dsigma + dxs)', 'hbm', None, B * T * D * 4 + B * L * T * 4 + 2 * B * L * D * 4 + 3 * B * L * 4
    if name in ('dx_upsample_prep', 'dx_upsample_sym_bwd'):
        return name[3:], 'hbm', None, 2 * a['B'] * a['L'] * a['D'] * 4 + 6 * a['B'] * a['L'] * 4
    if name in ('dx_adam_step', 'dx_adam_step_dyn'):
        return ('adam_kernel' if name == 'dx_adam_step' else 'adam_dyn_kernel'), 'hbm', None, a['n'] * 28
    if name == 'dx_scaler_update':                       # one lane: the eight state words read and written, the squared norm read
        return 'scaler_update', 'hbm', None, 2 * 8 * 4 + 4
    if name == 'dx_sumsq':
        return 'sumsq_kernel', 'hbm', None, a['n'] * 4
    if name == 'dx_mel_stats':
        return 'mel_stats', 'hbm', None, 2 * a['B'] * a['M'] * a['T'] * 4
    if name in ('dx_mel_grad', 'dx_mel_grad_dyn'):
        return 'mel_grad', 'hbm', None, 3 * a['B'] * a['M'] * a['T'] * 4
    if name == 'dx_add_pos':
        rows = geom.rows(a['B'], a['N'])
        return 'add_pos', 'hbm', None, rows * a['D'] * 4 * (2 if has('x') else 1)
    if name == 'dx_accent_sum':
        return 'accent_sum', 'hbm', None, geom.rows(a['B'], a['N']) * (2 * a['D'] * 4 + 8)
    if name == 'dx_scalar_conv_wgrad':
        return 'scalar_conv_wgrad', 'hbm', None, geom.rows(a['B'], a['N']) * (a['D'] * 4 if a['ldd'] else 0) + geom.rows(a['B'], a['N']) * 8
    if name == 'dx_transpose':
        return 'transpose', 'hbm', None, 2 * a['B'] * a['R'] * a['Cc'] * 4
    if name == 'dx_mask_rows':
        return 'mask_rows', 'hbm', None, 2 * geom.rows(a['B'], a['N']) * a['C'] * 4
    if name == 'dx_mean_pool':
        return 'mean_pool', 'hbm', None, geom.rows(a['B'], a['N']) * a['C'] * 4
    if name == 'dx_mean_pool_bwd':
        return 'mean_pool_bwd', 'hbm', None, geom.rows(a['B'], a['N']) * a['C'] * 4
    if name == 'dx_channel_affine':
        return 'channel_affine', 'hbm', None, 2 * a['rows'] * a['C'] * (2 if a.get('io_bf16') else 4)
    if name == 'dx_relu_bwd':
        return 'relu_bwd', 'hbm', None, 3 * a['n'] * 4
    if name == 'dx_colsum':
        return 'colsum', 'hbm', None, a['rows'] * a['C'] * (2 if a['x_bf16'] else 4)
    if name in ('dx_voc_conv_win', 'dx_voc_pair_win', 'dx_voc_chain_win', 'dx_voc_post_win', 'dx_voc_post_c_win'):   # the streaming forms: the rows of ONE interior window
        return price(name[:-4], dict(a, window_rows=a['B'] * a['step']), geom)  # (B x step; chunk 0 computes lag more, the last chunks fewer)
    if name == 'dx_voc_stream_advance':
        return 'voc_stream_advance', 'hbm', None, 8
    if name in ('dx_voc_conv', 'dx_voc_pair', 'dx_voc_chain', 'dx_voc_post', 'dx_voc_post_c'):   # HiFi-GAN vocoder: N rows of samples, frames * scale of them valid
        s = max(1, a['in_scale'] if name == 'dx_voc_conv' else a['scale'])
        rows = g('window_rows') or geom.rows(a['B'], a['N'] // s) * s
        op = ('f32', 'bf16', 'bf16x3')[g('bf16') or 0]          # the operand mode; 'bf16x3>' prices against a third of the bf16 peak
        if name == 'dx_voc_conv':                        # conv (up = 1) or polyphase transposed conv: rows in, rows * up out
            out_rows = rows * a['up']
            byt = rows * a['Cin'] * 4 + out_rows * a['Cout'] * 4 * (1 + has('R') + (a['acc_mode'] > 0))
            kind = 'voc_ups' if a['up'] > 1 else 'voc_pre' if a['Cin'] == 80 else 'voc_conv'
            return f'{kind}<{op}>', 'mfma', 2.0 * a['taps'] * a['Cin'] * a['Cout'] * out_rows, byt
        if name == 'dx_voc_pair':                        # two convs, X read, Y written (+ read when accumulating)
            return f'voc_pair<{op}>', 'mfma', 2.0 * 2 * a['taps'] * a['C'] * a['C'] * rows, rows * a['C'] * 4 * (2 + (a['acc_mode'] > 0))
        if name == 'dx_voc_chain':                       # a ResBlock2: two convs (the halo's recomputation is not credited), X read, Y written
            return f'voc_chain<{op}>', 'mfma', 2.0 * 2 * a['taps'] * a['C'] * a['C'] * rows, rows * a['C'] * 4 * (2 + (a['acc_mode'] > 0))
        return 'voc_post', 'hbm', None, rows * (a['C'] if name == 'dx_voc_post_c' else 32) * 4 + a['B'] * a['ncols'] * 4
    if name == 'dx_voc_wgrad':                           # generator training: both operands read once per tap, N rows, frames * scale valid
        s = max(1, a['scale'])
        rows = geom.rows(a['B'], a['N'] // s) * s
        k = 2 * a['up'] if a['up'] > 1 else a['taps']
        byt = rows * k * (a['Cin'] + a['Cout']) * 4 + a['Cout'] * a['Cin'] * k * 4
        return 'voc_wgrad<f32>', 'mfma', 2.0 * k * a['Cin'] * a['Cout'] * rows, byt
    if name == 'dx_voc_act_bwd':                         # U read, dX written, Xs / R / dX read when present
        return 'voc_act_bwd', 'hbm', None, a['B'] * a['N'] * a['C'] * 4 * (2 + has('Xs') + has('R') + (a['acc'] > 0))
    if name == 'dx_voc_post_bwd':                        # X read, dX written, Y and dY read
        return 'voc_post_bwd', 'hbm', None, a['B'] * a['N'] * (2 * a['C'] + 2) * 4
    if name == 'dx_voc_pack':
        return 'voc_pack', 'hbm', None, a['Cout'] * a['Cin'] * a['taps'] * max(1, a['up']) * (4 + (2 if a['bf16'] == 1 else 4))
    if name == 'dx_disc_conv':                           # HiFi-GAN discriminators: rows of N positions, no lengths
        nout = (a['N'] + 2 * a['pad'] - a['taps']) // a['stride'] + 1
        cin_g = a['Cin'] // a['groups']
        op = 'bf16' if g('bf16') else 'f32'
        byt = a['rows'] * (a['N'] * a['Cin'] + nout * a['Cout']) * 4 + a['Cout'] * cin_g * a['taps'] * (2 if g('bf16') else 4)
        kind = 'disc_conv_grouped' if a['groups'] > 1 else 'disc_conv'
        return f'{kind}<{op}>', 'mfma', 2.0 * a['rows'] * nout * a['taps'] * cin_g * a['Cout'], byt
    if name == 'dx_disc_first':                          # Cin = 1: the waveform read once, the feature map written once
        h = -(-a['T'] // a['p'])
        hout = (h + 2 * a['pad'] - a['taps']) // a['stride'] + 1
        return 'disc_first', 'hbm', None, a['B'] * (a['T'] + hout * a['p'] * a['Cout']) * 4
    if name == 'dx_disc_post':
        return 'disc_post', 'hbm', None, a['rows'] * a['N'] * (a['C'] + 1) * 4
    if name == 'dx_disc_pool':
        return 'disc_pool', 'hbm', None, a['R'] * (a['T'] + a['T'] // 2 + 1) * 4
    if name == 'dx_disc_losses':                         # both tensors of every entry read once
        return 'disc_losses', 'hbm', None, 2 * a['total_count'] * 4 + (3 * a['n_sets'] + 3 * a['n']) * 4
    if name == 'dx_disc_pack':
        return 'disc_pack', 'hbm', None, a['Cout'] * a['Cin_g'] * a['taps'] * (4 + (2 if a['bf16'] else 4))
    if name == 'dx_disc_conv_dgrad':                     # the forward layer's FLOPs for the same rows; dZ read, dX written, R and G read by the epilogue
        nout = (a['N'] + 2 * a['pad'] - a['taps']) // a['stride'] + 1
        cin_g = a['Cin'] // a['groups']
        op = 'bf16' if g('bf16') else 'f32'
        byt = a['rows'] * (nout * a['Cout'] + a['N'] * a['Cin'] * (3 if g('epilogue') else 1)) * 4 + a['Cout'] * cin_g * a['taps'] * (2 if g('bf16') else 4)
        kind = 'disc_dgrad_grouped' if a['groups'] > 1 else 'disc_dgrad'
        return f'{kind}<{op}>', 'mfma', 2.0 * a['rows'] * nout * a['taps'] * cin_g * a['Cout'], byt
    if name == 'dx_disc_post_bwd':                       # both score halves read, dZ written, R and G read
        return 'disc_post_bwd', 'hbm', None, a['rows'] * a['N'] * (2 + a['C'] * (3 if g('epilogue') else 1)) * 4
    if name == 'dx_disc_first_bwd':                      # dZ read once, the waveform gradient written (and read when accumulating)
        h = -(-a['T'] // a['p'])
        hout = (h + 2 * a['pad'] - a['taps']) // a['stride'] + 1
        return 'disc_first_bwd', 'hbm', None, a['B'] * (hout * a['p'] * a['Cout'] + a['T'] * (2 if g('accumulate') else 1)) * 4
    if name == 'dx_disc_pool_bwd':
        return 'disc_pool_bwd', 'hbm', None, a['R'] * (a['T'] // 2 + 1 + a['T'] * (2 if g('accumulate') else 1)) * 4
    if name == 'dx_disc_dgrad_pack':
        return 'disc_dgrad_pack', 'hbm', None, a['Cout'] * (a['Cin'] // a['groups']) * a['taps'] * (4 + (2 if a['bf16'] else 4))
    if name == 'dx_disc_wgrad':                          # the forward layer's FLOPs; A and dZ read once per tap group at best, G written
        nout = (a['N'] + 2 * a['pad'] - a['taps']) // a['stride'] + 1
        cin_g = a['Cin'] // a['groups']
        byt = a['rows'] * (a['N'] * a['Cin'] + nout * a['Cout']) * 4 + a['Cout'] * (cin_g * a['taps'] + 1) * 4
        kind = 'disc_wgrad_grouped' if a['groups'] > 1 else 'disc_wgrad'
        return f'{kind}<f32>', 'mfma', 2.0 * a['rows'] * nout * a['taps'] * cin_g * a['Cout'], byt
    if name == 'dx_disc_post_wgrad':                     # the scores and the last map read, dZ written, the map read again for dW
        return 'disc_post_wgrad', 'hbm', None, a['rows'] * a['N'] * (1 + 3 * a['C']) * 4
    if name == 'dx_disc_first_wgrad':                    # dZ and the waveform read once
        h = -(-a['T'] // a['p'])
        hout = (h + 2 * a['pad'] - a['taps']) // a['stride'] + 1
        return 'disc_first_wgrad', 'hbm', None, a['R'] * (hout * a['p'] * a['Cout'] + a['T']) * 4
    if name in ('dx_wn_adamw', 'dx_wn_fold'):            # the job table is in device memory: its owner logged the element counts
        from . import vocoder_optim
        normed, plain = vocoder_optim.TABLE_LOG.get(a['table'], (None, None))
        if normed is None:
            return name[3:], 'hbm', None, None
        if name == 'dx_wn_fold':                         # v read, W written
            return 'wn_fold', 'hbm', None, normed * 8
        return 'wn_adamw', 'hbm', None, normed * 32 + plain * 28      # dW, v, m, s read; v, m, s (and W) written
    if name == 'dx_mel':                                 # valid frames only: DFT GEMM (2 kmax outputs of 1024) + mel GEMM per frame
        frames = geom.rows(a['B'], a['T_max'])
        flops = 2.0 * frames * (1024 * 2 * a['kmax'] + a['kmax'] * a['n_mels'])
        return 'mel<f32>', 'mfma', flops, frames * (256 * 4 + (a['n_mels'] + 1) * 4)
    if name == 'dx_mel_bwd':                             # valid frames only: the forward's two GEMMs recomputed + their two transposes
        frames = geom.rows(a['B'], a['T_max'])
        flops = 2.0 * frames * 2 * (1024 * 2 * a['kmax'] + a['kmax'] * a['n_mels'])
        return 'mel_bwd<f32>', 'mfma', flops, frames * (2 * 256 * 4 + a['n_mels'] * 4)
    if name == 'dx_ft_batch':                            # per row: int16 samples read, fp32 samples written, the mel crop read and written
        return 'ft_batch', 'hbm', None, a['B'] * (a['segment_size'] * (2 + 4) + a['n_mels'] * a['fps'] * 2 * 4)
    if name in ('dx_mel_pack', 'dx_mel_bwd_pack'):
        return name[3:], 'hbm', None, a['n_mels'] * a['n_freq'] * 4 + (2 * 1024 + a['n_mels']) * a['kmax'] * 4
    if name == 'dx_symbol_prosody':                      # two frame rows in, int64 durations in, two symbol rows out
        return 'symbol_prosody', 'hbm', None, a['B'] * (2 * a['T'] * 4 + a['L'] * (8 + 2 * 4))
    if name == 'dx_prosody_condition':                   # energy, pitch, two factor rows in, int64 durations in, two rows out
        return 'prosody_condition', 'hbm', None, a['B'] * a['L'] * (6 * 4 + 8)
    if name == 'dx_pcm16':
        return 'pcm16', 'hbm', None, a['B'] * a['S'] * (4 + 2)
    if name == 'dx_gl_iter':                             # per valid frame: 513 magnitudes in, one hop of signal in and out
        frames = geom.rows(a['B'], a['T_max'])
        return 'gl_iter', 'hbm', None, frames * (513 * 4 + 2 * 256 * 4)
    if name == 'dx_gl_peak_normalize':
        return 'gl_peak_normalize', 'hbm', None, a['B'] * a['S'] * 3 * 4
    if name == 'dx_nnls_mel':
        frames = geom.rows(a['B'], a['T'])
        return 'nnls_mel', 'hbm', None, frames * (a['n_mels'] + 513) * 4
    return name[3:], 'hbm', None, None


def summarize(records, geom: Geometry, precision: str):
    """records of ONE step -> OrderedDict kernel label -> {launches, total_us, avg_us, bound, achieved, unit, peak, frac, ...},
    sorted by total time.  Events must have completed (synchronise first)."""
    rows = {}
    for name, args, ev0, ev1 in records:
        label, bound, flops, byt = price(name, args, geom)
        e = rows.setdefault(label, {'launches': 0, 'total_us': 0.0, 'bound': bound, 'flops': 0.0, 'bytes': 0.0, 'unpriced': 0})
        e['launches'] += 1
        e['total_us'] += ev0.elapsed_time(ev1) * 1e3
        if bound == 'mfma' and flops is not None:
            e['flops'] += flops
        if byt is not None:
            e['bytes'] += byt
        else:
            e['unpriced'] += 1
    out = OrderedDict()
    for label, e in sorted(rows.items(), key=lambda kv: -kv[1]['total_us']):
        t = e['total_us'] * 1e-6
        r = {'launches': e['launches'], 'total_us': round(e['total_us'], 1), 'avg_us': round(e['total_us'] / e['launches'], 2), 'bound': e['bound']}
        if e['bound'] == 'mfma':
            peak = PEAK_TFLOPS['bf16x3' if 'bf16x3>' in label else 'f32' if '<f32>' in label or precision in ('f32', 'bf16x3') else 'bf16']
            r.update(achieved=round(e['flops'] / t / 1e12, 2), unit='TFLOP/s', peak=peak, frac=round(e['flops'] / t / 1e12 / peak, 4),
                     algorithmic_bytes_per_launch=int(e['bytes'] / e['launches']))
        elif e['unpriced'] == 0:
            r.update(achieved=round(e['bytes'] / t / 1e9, 1), unit='GB/s', peak=PEAK_HBM_GBS, frac=round(e['bytes'] / t / 1e9 / PEAK_HBM_GBS, 4),
                     algorithmic_bytes_per_launch=int(e['bytes'] / e['launches']))
        out[label] = r
    return out
