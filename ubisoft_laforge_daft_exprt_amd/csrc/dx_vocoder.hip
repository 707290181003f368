// HiFi-GAN generators V1, V2 and V3 (reference src/daft_exprt/vocoder/hifigan.py) for inference: mel (B, 80, T) -> waveform (B, 256 T).
//
// Every convolution of the generator is one MFMA GEMM over a tile of 64 output samples of ONE batch row:
//   out[m][n] = sum_t sum_c A[m - pad + t*dil][c] * W[t][c][n]
// A is the input window staged in LDS (64 channels per chunk, leaky-ReLU prologue applied while staging, rows outside the row's
// valid length read as zero), W a pack of dx_voc_pack read fragment by fragment from L2.  Exact-f32 mode: v_mfma_f32_16x16x4_f32
// (four per 16-wide k step, each lane's float4 holds k = 4g..4g+3); bf16 mode: v_mfma_f32_16x16x32_bf16 (lane (row, g) holds
// k = 8g..8g+7), fp32 accumulation, fp32 storage between layers.  A and B use the same k map, so any permutation inside a step cancels.
// Split-bf16 mode (operand mode 2): bf16's k map on a hi and a lo bf16 image of every operand (x = hi + lo, dx_common.h); a product is
// hi*lo + lo*hi + hi*hi, three bf16 MFMAs, fp32 accumulation.  Activations are split while staging (after the fp32 leaky-ReLU), the
// pair's intermediate when it is written to LDS, the weights ONCE by dx_voc_pack: no conv kernel splits a weight.
//
// Valid lengths.  Every launch takes frames[b] (device int32) and the samples per frame of its input; rows of batch row b at or
// past frames[b] * scale do not exist: they are the conv's zero padding when read and are written as 0.  Tiles start at sample 0 of
// each batch row and every output element is summed in a fixed order, so batch row b is bitwise what the same row computes alone.
//
// The transposed convolutions (k = 2u, stride u, padding u/2) run in polyphase form: output sample s*u + r is a 2-tap conv of
// input samples s + base_r, s + base_r + 1 (base_r = -1 if r + u/2 < u else 0) with the phase's own 2 x Cin x Cout slice of W;
// grid.z = phase.  ResBlock1 pairs (conv dil d -> conv dil 1) of the 64- and 32-channel stages run fused (dx_voc_pair): the
// intermediate stays in LDS with its halo.
//
// Windowed form (template <bool WIN>, the dx_voc_*_win entry points): the streaming generator.  A launch reads the chunk index c from
// device memory and computes rows [lo, hi) = [c == 0 ? 0 : c step + lag, (c + 1) step + lag), clipped by the row's length, of its
// output; tiles start at lo.  Tensors live in rings: row n at slot n & mask (mask -1: plain indexing).  Every store and every
// read-modify-write is masked to [lo, hi), because a slot outside the window holds an older row that a later launch still reads; for
// the same reason nothing is zero-filled.  The zero padding at an utterance's two ends stays the 0 <= n < len test on LOGICAL rows.
// An output element is summed in an order that does not depend on where its tile starts, so a window writes the bits the whole call does.
#include "dx_common.h"

namespace {

constexpr float VOC_SLOPE = 0.1f;
constexpr int VT = 64;          // output samples per tile (4 MFMA row blocks)
constexpr int KC = 64;          // input channels per LDS chunk
constexpr int MIDR = 80;        // rows of the fused pair's intermediate: 64 + 2 * halo (halo <= 5), rounded up to 16
constexpr int THREADS = 256;

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * VOC_SLOPE; }

struct WinArgs {
  const int* cursor;      // device int32: the chunk index
  int step, lag;          // in tile rows
  int mx, my, mr;         // ring masks of X, Y, R (-1: plain indexing)
};

// rows [lo, hi) of the tile-row axis this launch computes, hi clipped by the valid length
template <bool WIN>
__device__ __forceinline__ void voc_window(const WinArgs& w, int len, int& lo, int& hi) {
  lo = 0;
  hi = len;
  if (WIN) {
    const int c = *w.cursor;
    lo = c == 0 ? 0 : c * w.step + w.lag;
    hi = min((c + 1) * w.step + w.lag, len);
  }
}

// A[rr][cc] = lrelu?(X[b][row0 + rr][c0 + cc]) for rr < R, cc < kcw; 0 outside [0, len) x [0, Cin).  Channels-last rows (sxc == 1,
// sxn >= Cin) are read as float4; any other layout (the (B, 80, T) mel, whose channel stride is 1 too when T == 1) element-wise.
// WIN: row n is read from ring slot n & mask.
// Mode 2: the hi image at A, the lo image los elements further on.
template <int MODE, bool WIN>
__device__ __forceinline__ void voc_stage(typename DxMmaMode<MODE>::T* A, int lda, int los, int R, const float* X, long sxn, long sxc,
                                          int row0, int len, int c0, int kcw, int Cin, int pro, int mask) {
  typedef DxMmaMode<MODE> Op;
  if (sxc == 1 && sxn >= Cin) {
    const int q = kcw >> 2;
    for (int e = threadIdx.x; e < R * q; e += THREADS) {
      const int rr = e / q, cc = (e - rr * q) * 4, n = row0 + rr, c = c0 + cc;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n >= 0 && n < len && c < Cin) {
        v = *reinterpret_cast<const float4*>(X + (long)(WIN ? n & mask : n) * sxn + c);
        if (pro) { v.x = lrelu(v.x); v.y = lrelu(v.y); v.z = lrelu(v.z); v.w = lrelu(v.w); }
      }
      Op::put4(A + rr * lda + cc, los, v);
    }
  } else {
    for (int e = threadIdx.x; e < R * kcw; e += THREADS) {
      const int cc = e / R, rr = e - cc * R, n = row0 + rr, c = c0 + cc;
      float v = 0.f;
      if (n >= 0 && n < len && c < Cin) {
        v = X[(long)(WIN ? n & mask : n) * sxn + (long)c * sxc];
        if (pro) v = lrelu(v);
      }
      Op::put(A + rr * lda + cc, los, v);
    }
  }
}

// acc[i][j] += sum_t sum_{k step s < nks} A[(16 mb_j + row + t*dil)][s*KS ...] * W[t][nb_i][ks0 + s]
// wave (wn, wm) owns column blocks nb_i = wn + i*WN and row blocks mb_j = wm + j*WM (< MB).
// Wp holds IMG 16-byte fragments per lane and step, back to back; A's lo image (mode 2) is los elements past A.  The fragments are
// loaded by plain statements over the images, not through the trait: the one-image instantiations then compile to what they did
// before there was a second image.
template <int MODE, int NI, int MI>
__device__ __forceinline__ void voc_mma(const typename DxMmaMode<MODE>::T* A, int lda, int los, int MB, int taps, int dil, const uint4* Wp,
                                        int NB, int KST, int ks0, int nks, int wn, int WN, int wm, int WM, f32x4 (&acc)[NI][MI]) {
  typedef DxMmaMode<MODE> Op;
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  for (int t = 0; t < taps; ++t) {
    for (int s = 0; s < nks; ++s) {
      uint4 b[NI][Op::IMG];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int m = 0; m < Op::IMG; ++m) b[i][m] = Wp[(((long)(t * NB + wn + i * WN) * KST + ks0 + s) * 64 + lane) * Op::IMG + m];
#pragma unroll
      for (int j = 0; j < MI; ++j) {
        const int mb = wm + j * WM;
        if (mb < MB) {
          uint4 a[Op::IMG];
#pragma unroll
          for (int m = 0; m < Op::IMG; ++m)
            a[m] = *reinterpret_cast<const uint4*>(A + m * los + (mb * 16 + r + t * dil) * lda + s * Op::KS + g * Op::VEC);
#pragma unroll
          for (int i = 0; i < NI; ++i) acc[i][j] = Op::mma(a, b[i], acc[i][j]);
        }
      }
    }
  }
}

__device__ __forceinline__ float voc_finish(float v, const float* y, int acc_mode) {
  if (acc_mode == 1) return *y + v;
  if (acc_mode == 2) return (*y + v) / 3.0f;
  return v;
}

struct ConvArgs {
  const float* X; long sxb, sxn, sxc;
  const uint4* Wp; const float* bias;
  float* Y; long syb; const float* R; long srb;
  const int* frames; int in_scale;
  int N, Cin, Cout, taps, dil, pad, up, KST, pro, acc_mode;
};

// One conv (up == 1) or one phase of a transposed conv (up > 1, grid.z = phase) on a 64-sample tile of one batch row.
template <int MODE, int NI, int MI, bool WIN>
__global__ void __launch_bounds__(THREADS) voc_conv_kernel(ConvArgs p, WinArgs win) {
  typedef DxMmaMode<MODE> Op;
  typedef typename Op::T T;
  extern __shared__ __attribute__((aligned(16))) unsigned char voc_smem[];
  T* A = reinterpret_cast<T*>(voc_smem);
  const int b = blockIdx.y, ph = blockIdx.z;
  const int in_len = min(p.frames[b] * p.in_scale, p.N);
  const int out_len = in_len * p.up;
  int lo, hi;
  voc_window<WIN>(win, in_len, lo, hi);
  const int m0 = lo + blockIdx.x * VT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  float* Y = p.Y + b * p.syb;
  const int NB = p.Cout / 16;
  const int WN = NB < 4 ? NB : 4, WM = 4 / WN, wn = w % WN, wm = w / WN;
  if (WIN) {
    if (m0 >= hi) return;                            // a tile wholly outside the window stores nothing
  } else if (m0 * p.up + ph >= out_len) {            // no valid output row in this tile: zeros only
    for (int e = threadIdx.x; e < VT * p.Cout; e += THREADS) {
      const int m = m0 + e / p.Cout, n = e % p.Cout;
      if (m < p.N) Y[(long)(m * p.up + ph) * p.Cout + n] = 0.f;
    }
    return;
  }
  int pad = p.pad;
  const uint4* Wp = p.Wp;
  if (p.up > 1) {
    pad = (ph + p.up / 2 < p.up) ? 1 : 0;
    Wp += (long)ph * 2 * NB * p.KST * 64 * Op::IMG;
  }
  const int rows = VT + (p.taps - 1) * p.dil, lda = KC + Op::PAD, los = rows * lda;
  const float* X = p.X + b * p.sxb;
  f32x4 acc[NI][MI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int KP = p.KST * Op::KS;
  for (int c0 = 0; c0 < KP; c0 += KC) {
    const int kcw = min(KC, KP - c0);
    __syncthreads();
    voc_stage<MODE, WIN>(A, lda, los, rows, X, p.sxn, p.sxc, m0 - pad, in_len, c0, kcw, p.Cin, p.pro, win.mx);
    __syncthreads();
    voc_mma<MODE, NI, MI>(A, lda, los, 4, p.taps, p.dil, Wp, NB, p.KST, c0 / Op::KS, kcw / Op::KS, wn, WN, wm, WM, acc);
  }
  const float* R = p.R ? p.R + b * p.srb : nullptr;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = (wn + i * WN) * 16 + r;
    const float bn = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int j = 0; j < MI; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + (wm + j * WM) * 16 + 4 * g + e;
        if (WIN) {                                   // only rows of the window, at their ring slots
          if (m >= hi) continue;
          const int row = m * p.up + ph;
          const long o = (long)(row & win.my) * p.Cout + n;
          float v = acc[i][j][e] + bn;
          if (R) v += R[(long)(row & win.mr) * p.Cout + n];
          Y[o] = voc_finish(v, Y + o, p.acc_mode);
          continue;
        }
        if (m >= p.N) continue;
        const long o = (long)(m * p.up + ph) * p.Cout + n;
        float v = 0.f;
        if (m * p.up + ph < out_len) {
          v = acc[i][j][e] + bn;
          if (R) v += R[o];
          v = voc_finish(v, Y + o, p.acc_mode);
        }
        Y[o] = v;
      }
    }
  }
}

struct PairArgs {
  const float* X; long sxb;
  const uint4* W1; const float* b1; const uint4* W2; const float* b2;
  float* Y; long syb;
  const int* frames; int scale;
  int N, C, taps, dil, KST, acc_mode;
};

// Y = acc_mode( conv2(lrelu(conv1(lrelu(X)) + b1)) + b2 + X ): one ResBlock1 pair, intermediate (80 rows with halo) in LDS.
// LDS: A's images, then M's (mode 2: A hi, A lo, M hi, M lo).
template <int MODE, int MI1, int MI2, bool WIN>
__global__ void __launch_bounds__(THREADS) voc_pair_kernel(PairArgs p, WinArgs win) {
  typedef DxMmaMode<MODE> Op;
  typedef typename Op::T T;
  extern __shared__ __attribute__((aligned(16))) unsigned char voc_smem[];
  const int b = blockIdx.y, C = p.C;
  const int len = min(p.frames[b] * p.scale, p.N);
  int lo, hi;
  voc_window<WIN>(win, len, lo, hi);
  const int s0 = lo + blockIdx.x * VT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  float* Y = p.Y + b * p.syb;
  if (WIN) {
    if (s0 >= hi) return;
  } else if (s0 >= len) {
    for (int e = threadIdx.x; e < VT * C; e += THREADS) {
      const int m = s0 + e / C;
      if (m < p.N) Y[(long)m * C + e % C] = 0.f;
    }
    return;
  }
  const int h2 = (p.taps - 1) / 2, h1 = p.dil * h2;
  // KP: C rounded up to whole K steps (C = 16 in bf16 mode is half a step: the pack holds zeros there, so A and M must hold zeros too)
  const int KP = p.KST * Op::KS;
  const int rows = MIDR + 2 * h1, lda = KC + Op::PAD, ldm = KP + Op::PAD, los = rows * lda, mos = MIDR * ldm;
  T* A = reinterpret_cast<T*>(voc_smem);
  T* M = A + Op::IMG * los;
  if (KP > C)                                        // columns C .. KP - 1 of M are operands too: zero (the first sync below orders this)
    for (int e = threadIdx.x; e < MIDR * ldm; e += THREADS) Op::put(M + e, mos, 0.f);
  const int NB = C / 16, WN = NB < 4 ? NB : 4, WM = 4 / WN, wn = w % WN, wm = w / WN;
  const float* X = p.X + b * p.sxb;
  f32x4 acc1[1][MI1];
#pragma unroll
  for (int j = 0; j < MI1; ++j) acc1[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < KP; c0 += KC) {
    const int kcw = min(KC, KP - c0);
    __syncthreads();
    voc_stage<MODE, WIN>(A, lda, los, rows, X, C, 1, s0 - h2 - h1, len, c0, kcw, C, 1, win.mx);
    __syncthreads();
    voc_mma<MODE, 1, MI1>(A, lda, los, MIDR / 16, p.taps, p.dil, p.W1, NB, p.KST, c0 / Op::KS, kcw / Op::KS, wn, WN, wm, WM, acc1);
  }
  {
    const int n = wn * 16 + r;
    const float bn = p.b1[n];
#pragma unroll
    for (int j = 0; j < MI1; ++j) {
      const int mb = wm + j * WM;
      if (mb < MIDR / 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = mb * 16 + 4 * g + e, s = s0 - h2 + q;
          Op::put(M + q * ldm + n, mos, (s >= 0 && s < len) ? lrelu(acc1[0][j][e] + bn) : 0.f);
        }
      }
    }
  }
  __syncthreads();
  f32x4 acc2[1][MI2];
#pragma unroll
  for (int j = 0; j < MI2; ++j) acc2[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  voc_mma<MODE, 1, MI2>(M, ldm, mos, VT / 16, p.taps, 1, p.W2, NB, p.KST, 0, p.KST, wn, WN, wm, WM, acc2);
  const int n = wn * 16 + r;
  const float bn = p.b2[n];
#pragma unroll
  for (int j = 0; j < MI2; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = s0 + (wm + j * WM) * 16 + 4 * g + e;
      if (WIN) {
        if (m >= hi) continue;
        const long o = (long)(m & win.my) * C + n;
        Y[o] = voc_finish(acc2[0][j][e] + bn + X[(long)(m & win.mx) * C + n], Y + o, p.acc_mode);
        continue;
      }
      if (m >= p.N) continue;
      const long o = (long)m * C + n;
      float v = 0.f;
      if (m < len) v = voc_finish(acc2[0][j][e] + bn + X[o], Y + o, p.acc_mode);
      Y[o] = v;
    }
  }
}

struct ChainArgs {
  const float* X; long sxb;
  const uint4* W1; const float* b1; const uint4* W2; const float* b2;
  float* Y; long syb;
  const int* frames; int scale;
  int N, C, taps, d1, d2, KST, acc_mode;
};

// One ResBlock2 (V3) in one launch: x1 = conv_d1(lrelu(X)) + b1 + X, Y = acc_mode( conv_d2(lrelu(x1)) + b2 + x1 ).
// x1 is computed on 64 + 2 HR rows, HR = the second conv's halo h2 = d2 (taps - 1) / 2 rounded up to 16, and never leaves the CU:
// lrelu(x1) goes to LDS as the second conv's operand (over the input window, which is dead by then) and the fp32 x1 stays in the
// accumulators.  Because HR is whole row blocks, the 64 central rows of x1 sit on the same lanes and elements as the output's, HR / 16
// row blocks further on: conv1 hands row blocks to the waves shifted by that many (wm1), so that the wave that owns an output block
// also owns its x1 block, and the second residual is the fp32 x1 in both precision modes.  Rows of x1 outside [0, len) are 0, as the
// two-conv form writes them.  Each sum runs taps-outer, K-steps-inner as in voc_conv_kernel, whatever the tile's start.
// Operand modes 0 and 1 only: the chain has no split form.
template <bool BF, int MI1, int MI2, bool WIN>
__global__ void __launch_bounds__(THREADS) voc_chain_kernel(ChainArgs p, WinArgs win) {
  typedef DxMmaMode<BF> Op;
  typedef typename Op::T T;
  extern __shared__ __attribute__((aligned(16))) unsigned char voc_smem[];
  const int b = blockIdx.y, C = p.C;
  const int len = min(p.frames[b] * p.scale, p.N);
  int lo, hi;
  voc_window<WIN>(win, len, lo, hi);
  const int s0 = lo + blockIdx.x * VT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  float* Y = p.Y + b * p.syb;
  if (WIN) {
    if (s0 >= hi) return;
  } else if (s0 >= len) {
    for (int e = threadIdx.x; e < VT * C; e += THREADS) {
      const int m = s0 + e / C;
      if (m < p.N) Y[(long)m * C + e % C] = 0.f;
    }
    return;
  }
  const int hk = (p.taps - 1) / 2, h1 = p.d1 * hk, h2 = p.d2 * hk;
  const int HR = (h2 + 15) & ~15, midr = VT + 2 * HR, MB1 = midr / 16;
  const int KP = p.KST * Op::KS;
  const int rows = midr + 2 * h1, lda = KC + Op::PAD, ldm = KP + Op::PAD;
  T* A = reinterpret_cast<T*>(voc_smem);
  T* M = A;                                          // lrelu(x1) overlays the input window once conv1 has read it
  const int NB = C / 16, WN = NB < 4 ? NB : 4, WM = 4 / WN, wn = w % WN, wm = w / WN;
  const int wm1 = (wm + HR / 16) % WM, joff = (wm + HR / 16 - wm1) / WM;     // x1 block wm1 + (joff + j) WM holds output block wm + j WM
  const float* X = p.X + b * p.sxb;
  f32x4 x1[1][MI1];
#pragma unroll
  for (int j = 0; j < MI1; ++j) x1[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < KP; c0 += KC) {
    const int kcw = min(KC, KP - c0);
    __syncthreads();
    voc_stage<BF, WIN>(A, lda, 0, rows, X, C, 1, s0 - HR - h1, len, c0, kcw, C, 1, win.mx);
    __syncthreads();
    voc_mma<BF, 1, MI1>(A, lda, 0, MB1, p.taps, p.d1, p.W1, NB, p.KST, c0 / Op::KS, kcw / Op::KS, wn, WN, wm1, WM, x1);
  }
  __syncthreads();                                   // every wave is done with A
  const int n = wn * 16 + r;
  {
    const float bn = p.b1[n];
#pragma unroll
    for (int j = 0; j < MI1; ++j) {
      const int mb = wm1 + j * WM;
      if (mb < MB1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = mb * 16 + 4 * g + e, s = s0 - HR + q;
          float v = 0.f;
          if (s >= 0 && s < len) v = x1[0][j][e] + bn + X[(long)(WIN ? s & win.mx : s) * C + n];
          x1[0][j][e] = v;
          M[q * ldm + n] = Op::cvt(lrelu(v));
        }
      }
    }
  }
  __syncthreads();
  f32x4 acc2[1][MI2];
#pragma unroll
  for (int j = 0; j < MI2; ++j) acc2[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  voc_mma<BF, 1, MI2>(M + (HR - h2) * ldm, ldm, 0, VT / 16, p.taps, p.d2, p.W2, NB, p.KST, 0, p.KST, wn, WN, wm, WM, acc2);
  const float bn = p.b2[n];
#pragma unroll
  for (int j2 = 0; j2 < MI2; ++j2) {
    f32x4 res = f32x4{0.f, 0.f, 0.f, 0.f};           // the fp32 x1 of this output block: a wave-uniform pick, no dynamic indexing
#pragma unroll
    for (int j = 0; j < MI1; ++j)
      if (j == joff + j2) res = x1[0][j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = s0 + (wm + j2 * WM) * 16 + 4 * g + e;
      if (WIN) {
        if (m >= hi) continue;
        const long o = (long)(m & win.my) * C + n;
        Y[o] = voc_finish(acc2[0][j2][e] + bn + res[e], Y + o, p.acc_mode);
        continue;
      }
      if (m >= p.N) continue;
      const long o = (long)m * C + n;
      float v = 0.f;
      if (m < len) v = voc_finish(acc2[0][j2][e] + bn + res[e], Y + o, p.acc_mode);
      Y[o] = v;
    }
  }
}

// conv_post (C -> 1, C = 32 or 16, k = 7, padding 3) on lrelu(X), then tanh and the clip to [-1, 1]; one output sample per thread.
// Y row b holds ncols samples: those at or past the row's valid length are written as 0.  WIN: sample s of the window goes to column
// s - c step of the chunk buffer.
template <bool WIN, int C>
__global__ void __launch_bounds__(THREADS) voc_post_kernel(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy,
                                                           const int* frames, int scale, int N, int ncols, WinArgs win) {
  __shared__ float ws[C * 7];
  for (int e = threadIdx.x; e < C * 7; e += THREADS) ws[e] = W[e];
  __syncthreads();
  const int b = blockIdx.y;
  const int len = min(frames[b] * scale, N);
  int s = blockIdx.x * THREADS + threadIdx.x, col = s;
  if (WIN) {
    const int c = *win.cursor;
    s += c == 0 ? 0 : c * win.step + win.lag;
    col = s - c * win.step;
    if (s >= (c + 1) * win.step + win.lag) return;
  }
  if (col >= ncols) return;
  float v = 0.f;
  if (s < len) {
    const float* x = X + b * sxb;
    float acc = 0.f;
    for (int t = 0; t < 7; ++t) {
      const int n = s - 3 + t;
      if (n < 0 || n >= len) continue;
      const float4* xr = reinterpret_cast<const float4*>(x + (long)(WIN ? n & win.mx : n) * C);
#pragma unroll
      for (int c4 = 0; c4 < C / 4; ++c4) {
        const float4 q = xr[c4];
        acc = __builtin_fmaf(lrelu(q.x), ws[(4 * c4 + 0) * 7 + t], acc);
        acc = __builtin_fmaf(lrelu(q.y), ws[(4 * c4 + 1) * 7 + t], acc);
        acc = __builtin_fmaf(lrelu(q.z), ws[(4 * c4 + 2) * 7 + t], acc);
        acc = __builtin_fmaf(lrelu(q.w), ws[(4 * c4 + 3) * 7 + t], acc);
      }
    }
    v = fminf(fmaxf(tanhf(acc + bias[0]), -1.f), 1.f);
  }
  Y[(long)b * ldy + col] = v;
}

// The chunk's last launch: the next replay of the same launches computes the next window.
__global__ void voc_advance_kernel(int* cursor) { *cursor += 1; }

// Pack: [phase][t][nb][ks][lane][IMG][VEC]; lane (n = l & 15, g = l >> 4) element v holds k = ks*KS + g*VEC + v of column nb*16 + n.
// Mode 2: a lane's eight hi = bf16_rne(w), then its eight lo = bf16_rne(w - hi) (0 where hi is not finite): 32 bytes per lane and
// step, the f32 pack's size wherever Cin is whole 32-deep steps.  The weights are split here, once.
// up == 1: W (Cout, Cin, taps); up > 1: W (Cin, Cout, 2 up) of a ConvTranspose1d, tap t of phase r = kernel index j0(r) - t*up.
template <int MODE>
__global__ void voc_pack_kernel(const float* W, void* out, int Cout, int Cin, int taps, int up, int KST, long total) {
  typedef DxMmaMode<MODE> Op;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int NB = Cout / 16, v = (int)(e % Op::VEC);
  long f = e / Op::VEC;
  const int img = (int)(f % Op::IMG); f /= Op::IMG;
  const int lane = (int)(f % 64); f /= 64;
  const int ks = (int)(f % KST); f /= KST;
  const int nb = (int)(f % NB); f /= NB;
  const int t = (int)(f % taps); f /= taps;
  const int ph = (int)f;
  const int k = ks * Op::KS + (lane >> 4) * Op::VEC + v, n = nb * 16 + (lane & 15);
  float val = 0.f;
  if (k < Cin) {
    if (up == 1) {
      val = W[((long)n * Cin + k) * taps + t];
    } else {
      const int q = ph + up / 2, j = (q < up ? q + up : q) - t * up;
      val = W[((long)k * Cout + n) * (2 * up) + j];
    }
  }
  typename Op::T o = (typename Op::T)val;
  if (img) {                                         // the lo image: what hi leaves of val
    const float hi = (float)o;
    o = (typename Op::T)(__builtin_isfinite(hi) ? val - hi : 0.f);
  }
  reinterpret_cast<typename Op::T*>(out)[e] = o;
}

// elements of a pack: 4 f32, 8 bf16 or 8 + 8 bf16 per lane and k step (mode 0, 1, 2)
long voc_pack_elems(int Cout, int Cin, int taps, int up, int mode) {
  const int KS = mode ? 32 : 16;
  return (long)(up > 1 ? up : 1) * taps * (Cout / 16) * dx_cdiv(Cin, KS) * 64 * (mode == 2 ? 16 : mode ? 8 : 4);
}

// win == nullptr: the whole tensor (tiles over N rows); else the window kernels, with a grid for chunk 0's window of step + lag rows.
template <int MODE, int NI, int MI>
int launch_conv(const ConvArgs& a, const WinArgs* win, int B, hipStream_t s) {
  typedef DxMmaMode<MODE> Op;
  const size_t smem = (size_t)(VT + (a.taps - 1) * a.dil) * (KC + Op::PAD) * Op::IMG * sizeof(typename Op::T);
  if (win)
    hipLaunchKernelGGL((voc_conv_kernel<MODE, NI, MI, true>), dim3(dx_cdiv(win->step + win->lag, VT), B, a.up), dim3(THREADS), smem, s, a, *win);
  else
    hipLaunchKernelGGL((voc_conv_kernel<MODE, NI, MI, false>), dim3(dx_cdiv(a.N, VT), B, a.up), dim3(THREADS), smem, s, a, WinArgs{});
  DX_LAUNCH_CHECK("dx_voc_conv");
  return DX_OK;
}

template <int MODE>
int dispatch_conv(const ConvArgs& a, const WinArgs* win, int B, hipStream_t s) {
  switch (a.Cout / 16) {
    case 32: return launch_conv<MODE, 8, 4>(a, win, B, s);
    case 16: return launch_conv<MODE, 4, 4>(a, win, B, s);
    case 8: return launch_conv<MODE, 2, 4>(a, win, B, s);
    case 4: return launch_conv<MODE, 1, 4>(a, win, B, s);
    case 1: return launch_conv<MODE, 1, 1>(a, win, B, s);      // 16 columns: one column block, the four waves over the four row blocks
    default: return launch_conv<MODE, 1, 2>(a, win, B, s);
  }
}

// LDS: 80 + 2 h1 rows of the input and 80 of the intermediate, in every image: at C = 64, taps 11, dilation 5 (130 rows) 57.1 KB in f32
// mode, 60.5 KB in mode 2 -- the largest of any launch, inside the 64 KB a launch gets without asking for more
template <int MODE, int MI1, int MI2>
int launch_pair(const PairArgs& a, const WinArgs* win, int B, hipStream_t s) {
  typedef DxMmaMode<MODE> Op;
  const int h1 = a.dil * (a.taps - 1) / 2;
  const size_t smem = ((size_t)(MIDR + 2 * h1) * (KC + Op::PAD) + (size_t)MIDR * (a.KST * Op::KS + Op::PAD)) * Op::IMG * sizeof(typename Op::T);
  if (win)
    hipLaunchKernelGGL((voc_pair_kernel<MODE, MI1, MI2, true>), dim3(dx_cdiv(win->step + win->lag, VT), B), dim3(THREADS), smem, s, a, *win);
  else
    hipLaunchKernelGGL((voc_pair_kernel<MODE, MI1, MI2, false>), dim3(dx_cdiv(a.N, VT), B), dim3(THREADS), smem, s, a, WinArgs{});
  DX_LAUNCH_CHECK("dx_voc_pair");
  return DX_OK;
}

// LDS: the input window, 64 + 2 HR + 2 h1 rows of 64 channels (x1's operand copy overlays it): 178 rows = 48.4 KB at most in f32 mode
template <bool BF, int MI1, int MI2>
int launch_chain(const ChainArgs& a, const WinArgs* win, int B, hipStream_t s) {
  typedef DxMmaMode<BF> Op;
  const int hk = (a.taps - 1) / 2, HR = (a.d2 * hk + 15) & ~15;
  const size_t smem = (size_t)(VT + 2 * HR + 2 * a.d1 * hk) * (KC + Op::PAD) * sizeof(typename Op::T);
  if (win)
    hipLaunchKernelGGL((voc_chain_kernel<BF, MI1, MI2, true>), dim3(dx_cdiv(win->step + win->lag, VT), B), dim3(THREADS), smem, s, a, *win);
  else
    hipLaunchKernelGGL((voc_chain_kernel<BF, MI1, MI2, false>), dim3(dx_cdiv(a.N, VT), B), dim3(THREADS), smem, s, a, WinArgs{});
  DX_LAUNCH_CHECK("dx_voc_chain");
  return DX_OK;
}

// A ring mask is 0 (plain indexing, passed to the kernels as -1) or 2^k - 1; the window is [c step + lag, (c + 1) step + lag).
bool voc_mask_ok(int m) { return m >= 0 && (m & (m + 1)) == 0; }
bool voc_win_ok(const void* cursor, int step, int lag, int mx, int my, int mr) {
  return cursor && step > 0 && lag >= 0 && voc_mask_ok(mx) && voc_mask_ok(my) && voc_mask_ok(mr);
}
WinArgs voc_win(const int* cursor, int step, int lag, int mx, int my, int mr) {
  WinArgs w;
  w.cursor = cursor; w.step = step; w.lag = lag;
  w.mx = mx ? mx : -1; w.my = my ? my : -1; w.mr = mr ? mr : -1;
  return w;
}

bool voc_taps_ok(int taps, int dil) { return (taps == 3 || taps == 7 || taps == 11) && (dil == 1 || dil == 3 || dil == 5); }

// dx_voc_conv (win == nullptr; srb = syb) and dx_voc_conv_win
int voc_conv(const float* X, long sxb, long sxn, long sxc, const void* Wp, const float* bias, float* Y, long syb, const float* R, long srb,
             const int* frames, int in_scale, int B, int N, int Cin, int Cout, int taps, int dil, int up, int lrelu_in, int acc_mode,
             int bf16, const WinArgs* win, void* stream) {
  DX_REQUIRE(X && Wp && Y && frames, "dx_voc_conv: null pointer");
  DX_REQUIRE(B > 0 && N > 0 && in_scale > 0 && Cin > 0 &&
                 (Cout == 16 || Cout == 32 || Cout == 64 || Cout == 128 || Cout == 256 || Cout == 512),
             "dx_voc_conv: bad shape (Cout in {16, 32, 64, 128, 256, 512})");
  // the LDS window is 64 + dil (taps - 1) rows of 64 channels: at most 136 rows, 37 KB in f32 mode, 39 KB in mode 2 (hi and lo images)
  DX_REQUIRE(up == 1 ? (taps >= 1 && taps % 2 == 1 && taps <= 11 && dil >= 1 && dil * (taps - 1) <= 72)
                     : (taps == 2 && dil == 1 && up >= 2 && up % 2 == 0 && up <= 8),
             "dx_voc_conv: bad taps / dilation / upsampling (odd taps <= 11 with dilation (taps - 1) <= 72, or a polyphase transposed conv: taps 2, even up <= 8)");
  DX_REQUIRE(acc_mode >= 0 && acc_mode <= 2 && bf16 >= 0 && bf16 <= 2, "dx_voc_conv: bad acc_mode / bf16 (operand mode 0, 1 or 2)");
  DX_REQUIRE((const void*)X != (const void*)Y, "dx_voc_conv: Y must not alias X (tiles read their neighbours' rows); R may alias Y");
  DX_REQUIRE(sxc != 1 || sxn < Cin || (Cin % 4 == 0 && sxn % 4 == 0 && sxb % 4 == 0 && ((uintptr_t)X & 15) == 0),
             "dx_voc_conv: channels-last input needs Cin and strides %% 4 == 0 and a 16-byte aligned X");
  ConvArgs a;
  a.X = X; a.sxb = sxb; a.sxn = sxn; a.sxc = sxc;
  a.Wp = reinterpret_cast<const uint4*>(Wp); a.bias = bias;
  a.Y = Y; a.syb = syb; a.R = R; a.srb = srb;
  a.frames = frames; a.in_scale = in_scale;
  a.N = N; a.Cin = Cin; a.Cout = Cout; a.taps = taps; a.dil = dil; a.pad = dil * (taps - 1) / 2; a.up = up;
  a.KST = dx_cdiv(Cin, bf16 ? 32 : 16); a.pro = lrelu_in; a.acc_mode = acc_mode;
  if (bf16 == 2) return dispatch_conv<2>(a, win, B, (hipStream_t)stream);
  return bf16 ? dispatch_conv<1>(a, win, B, (hipStream_t)stream) : dispatch_conv<0>(a, win, B, (hipStream_t)stream);
}

// dx_voc_pair (win == nullptr; syb = sxb) and dx_voc_pair_win
int voc_pair(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y, long syb,
             const int* frames, int scale, int B, int N, int C, int taps, int dil, int acc_mode, int bf16, const WinArgs* win, void* stream) {
  DX_REQUIRE(X && W1 && b1 && W2 && b2 && Y && frames, "dx_voc_pair: null pointer");
  DX_REQUIRE(X != Y, "dx_voc_pair: Y must not alias X (tiles read their neighbours' rows)");
  DX_REQUIRE(B > 0 && N > 0 && scale > 0 && (C == 16 || C == 32 || C == 64) && sxb % 4 == 0 && ((uintptr_t)X & 15) == 0,
             "dx_voc_pair: bad shape (C in {16, 32, 64}; sxb %% 4 == 0 and a 16-byte aligned X)");
  DX_REQUIRE(voc_taps_ok(taps, dil), "dx_voc_pair: bad taps / dilation (taps 3, 7 or 11; dilation 1, 3 or 5)");
  DX_REQUIRE(acc_mode >= 0 && acc_mode <= 2 && bf16 >= 0 && bf16 <= 2, "dx_voc_pair: bad acc_mode / bf16 (operand mode 0, 1 or 2)");
  PairArgs a;
  a.X = X; a.sxb = sxb;
  a.W1 = reinterpret_cast<const uint4*>(W1); a.b1 = b1; a.W2 = reinterpret_cast<const uint4*>(W2); a.b2 = b2;
  a.Y = Y; a.syb = syb; a.frames = frames; a.scale = scale;
  a.N = N; a.C = C; a.taps = taps; a.dil = dil; a.KST = dx_cdiv(C, bf16 ? 32 : 16); a.acc_mode = acc_mode;
  hipStream_t s = (hipStream_t)stream;
  if (bf16 == 2) return C == 16 ? launch_pair<2, 2, 1>(a, win, B, s) : C == 64 ? launch_pair<2, 5, 4>(a, win, B, s) : launch_pair<2, 3, 2>(a, win, B, s);
  if (C == 16) return bf16 ? launch_pair<1, 2, 1>(a, win, B, s) : launch_pair<0, 2, 1>(a, win, B, s);
  if (C == 64) return bf16 ? launch_pair<1, 5, 4>(a, win, B, s) : launch_pair<0, 5, 4>(a, win, B, s);
  return bf16 ? launch_pair<1, 3, 2>(a, win, B, s) : launch_pair<0, 3, 2>(a, win, B, s);
}

// dx_voc_chain (win == nullptr; syb = sxb) and dx_voc_chain_win
int voc_chain(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y, long syb,
              const int* frames, int scale, int B, int N, int C, int taps, int d1, int d2, int acc_mode, int bf16, const WinArgs* win,
              void* stream) {
  DX_REQUIRE(X && W1 && b1 && W2 && b2 && Y && frames, "dx_voc_chain: null pointer");
  DX_REQUIRE(X != Y, "dx_voc_chain: Y must not alias X (tiles read their neighbours' rows)");
  DX_REQUIRE(B > 0 && N > 0 && scale > 0 && (C == 32 || C == 64) && sxb % 4 == 0 && ((uintptr_t)X & 15) == 0,
             "dx_voc_chain: bad shape (C in {32, 64}; sxb %% 4 == 0 and a 16-byte aligned X)");
  // ten row blocks of x1 at most (HR <= 48), and an input window of at most 178 rows
  DX_REQUIRE((taps == 3 || taps == 5 || taps == 7) && d1 >= 1 && d2 >= 1 && d1 * (taps - 1) <= 18 && d2 * (taps - 1) <= 72,
             "dx_voc_chain: bad taps / dilation (taps 3, 5 or 7; d1 (taps - 1) <= 18, d2 (taps - 1) <= 72)");
  DX_REQUIRE(bf16 != 2, "dx_voc_chain: no split-bf16 form (operand mode 2): run the ResBlock2 as two dx_voc_conv launches");
  DX_REQUIRE(acc_mode >= 0 && acc_mode <= 2 && (bf16 == 0 || bf16 == 1), "dx_voc_chain: bad acc_mode / bf16");
  ChainArgs a;
  a.X = X; a.sxb = sxb;
  a.W1 = reinterpret_cast<const uint4*>(W1); a.b1 = b1; a.W2 = reinterpret_cast<const uint4*>(W2); a.b2 = b2;
  a.Y = Y; a.syb = syb; a.frames = frames; a.scale = scale;
  a.N = N; a.C = C; a.taps = taps; a.d1 = d1; a.d2 = d2; a.KST = C / (bf16 ? 32 : 16); a.acc_mode = acc_mode;
  hipStream_t s = (hipStream_t)stream;
  if (C == 64) return bf16 ? launch_chain<true, 10, 4>(a, win, B, s) : launch_chain<false, 10, 4>(a, win, B, s);
  return bf16 ? launch_chain<true, 5, 2>(a, win, B, s) : launch_chain<false, 5, 2>(a, win, B, s);
}

}  // namespace

extern "C" {

int dx_voc_pack_size(int Cout, int Cin, int taps, int up, int bf16, long* bytes) {
  DX_REQUIRE(bytes, "dx_voc_pack_size: null output");
  DX_REQUIRE(Cout > 0 && Cout % 16 == 0 && Cin > 0 && taps > 0 && up >= 1 && (up == 1 || taps == 2) && bf16 >= 0 && bf16 <= 2,
             "dx_voc_pack_size: bad shape (Cout %% 16 == 0; a transposed conv (up > 1) has taps = 2 in polyphase form; operand mode 0, 1 or 2)");
  *bytes = voc_pack_elems(Cout, Cin, taps, up, bf16) * (bf16 ? 2 : 4);
  return DX_OK;
}

int dx_voc_pack(const float* W, void* Wp, int Cout, int Cin, int taps, int up, int bf16, void* stream) {
  DX_REQUIRE(W && Wp, "dx_voc_pack: null pointer");
  DX_REQUIRE(Cout > 0 && Cout % 16 == 0 && Cin > 0 && taps > 0 && up >= 1 && (up == 1 || (taps == 2 && up % 2 == 0)) && bf16 >= 0 && bf16 <= 2,
             "dx_voc_pack: bad shape (Cout %% 16 == 0; a transposed conv (up > 1, even) has taps = 2 in polyphase form; operand mode 0, 1 or 2)");
  const long total = voc_pack_elems(Cout, Cin, taps, up, bf16);
  const int KST = dx_cdiv(Cin, bf16 ? 32 : 16);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (bf16 == 2)
    hipLaunchKernelGGL(voc_pack_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cout, Cin, taps, up, KST, total);
  else if (bf16)
    hipLaunchKernelGGL(voc_pack_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cout, Cin, taps, up, KST, total);
  else
    hipLaunchKernelGGL(voc_pack_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cout, Cin, taps, up, KST, total);
  DX_LAUNCH_CHECK("dx_voc_pack");
  return DX_OK;
}

int dx_voc_conv(const float* X, long sxb, long sxn, long sxc, const void* Wp, const float* bias, float* Y, long syb, const float* R,
                const int* frames, int in_scale, int B, int N, int Cin, int Cout, int taps, int dil, int up, int lrelu_in, int acc_mode,
                int bf16, void* stream) {
  return voc_conv(X, sxb, sxn, sxc, Wp, bias, Y, syb, R, syb, frames, in_scale, B, N, Cin, Cout, taps, dil, up, lrelu_in, acc_mode, bf16,
                  nullptr, stream);
}

int dx_voc_conv_win(const float* X, long sxb, long sxn, long sxc, const void* Wp, const float* bias, float* Y, long syb, const float* R,
                    long srb, const int* frames, int in_scale, int B, int N, int Cin, int Cout, int taps, int dil, int up, int lrelu_in,
                    int acc_mode, int bf16, const int* cursor, int step, int lag, int mx, int my, int mr, void* stream) {
  DX_REQUIRE(voc_win_ok(cursor, step, lag, mx, my, mr), "dx_voc_conv_win: bad window (cursor, step > 0, lag >= 0, masks 0 or 2^k - 1)");
  DX_REQUIRE(my == 0 || (long)(my + 1) * Cout <= syb, "dx_voc_conv_win: Y's ring does not fit its batch stride");
  DX_REQUIRE(!R || (mr ? (long)(mr + 1) : (long)N * (up > 1 ? up : 1)) * Cout <= srb, "dx_voc_conv_win: R's ring (or its N rows) does not fit its batch stride");
  DX_REQUIRE(mx == 0 || (long)mx * sxn + (long)(Cin - 1) * sxc < sxb, "dx_voc_conv_win: X's ring does not fit its batch stride");
  DX_REQUIRE(my != 0 || (long)N * (up > 1 ? up : 1) * Cout <= syb, "dx_voc_conv_win: an unringed Y holds all N rows");
  const WinArgs w = voc_win(cursor, step, lag, mx, my, mr);
  return voc_conv(X, sxb, sxn, sxc, Wp, bias, Y, syb, R, srb, frames, in_scale, B, N, Cin, Cout, taps, dil, up, lrelu_in, acc_mode, bf16,
                  &w, stream);
}

int dx_voc_pair(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y,
                const int* frames, int scale, int B, int N, int C, int taps, int dil, int acc_mode, int bf16, void* stream) {
  return voc_pair(X, sxb, W1, b1, W2, b2, Y, sxb, frames, scale, B, N, C, taps, dil, acc_mode, bf16, nullptr, stream);
}

int dx_voc_pair_win(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y, long syb,
                    const int* frames, int scale, int B, int N, int C, int taps, int dil, int acc_mode, int bf16, const int* cursor,
                    int step, int lag, int mx, int my, void* stream) {
  DX_REQUIRE(voc_win_ok(cursor, step, lag, mx, my, 0), "dx_voc_pair_win: bad window (cursor, step > 0, lag >= 0, masks 0 or 2^k - 1)");
  DX_REQUIRE((mx ? (long)(mx + 1) : (long)N) * C <= sxb && (my ? (long)(my + 1) : (long)N) * C <= syb,
             "dx_voc_pair_win: a ring (or the N rows of an unringed tensor) does not fit its batch stride");
  const WinArgs w = voc_win(cursor, step, lag, mx, my, 0);
  return voc_pair(X, sxb, W1, b1, W2, b2, Y, syb, frames, scale, B, N, C, taps, dil, acc_mode, bf16, &w, stream);
}

int dx_voc_chain(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y,
                 const int* frames, int scale, int B, int N, int C, int taps, int d1, int d2, int acc_mode, int bf16, void* stream) {
  return voc_chain(X, sxb, W1, b1, W2, b2, Y, sxb, frames, scale, B, N, C, taps, d1, d2, acc_mode, bf16, nullptr, stream);
}

int dx_voc_chain_win(const float* X, long sxb, const void* W1, const float* b1, const void* W2, const float* b2, float* Y, long syb,
                     const int* frames, int scale, int B, int N, int C, int taps, int d1, int d2, int acc_mode, int bf16,
                     const int* cursor, int step, int lag, int mx, int my, void* stream) {
  DX_REQUIRE(voc_win_ok(cursor, step, lag, mx, my, 0), "dx_voc_chain_win: bad window (cursor, step > 0, lag >= 0, masks 0 or 2^k - 1)");
  DX_REQUIRE(C > 0 && (mx ? (long)(mx + 1) : (long)N) * C <= sxb && (my ? (long)(my + 1) : (long)N) * C <= syb,
             "dx_voc_chain_win: a ring (or the N rows of an unringed tensor) does not fit its batch stride");
  const WinArgs w = voc_win(cursor, step, lag, mx, my, 0);
  return voc_chain(X, sxb, W1, b1, W2, b2, Y, syb, frames, scale, B, N, C, taps, d1, d2, acc_mode, bf16, &w, stream);
}

int dx_voc_post_c(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                  int B, int N, int ncols, int C, void* stream) {
  DX_REQUIRE(X && W && bias && Y && frames, "dx_voc_post: null pointer");
  DX_REQUIRE(C == 16 || C == 32, "dx_voc_post: bad channel count (C in {16, 32})");
  DX_REQUIRE(B > 0 && N > 0 && scale > 0 && ncols >= N && ldy >= ncols && sxb % 4 == 0 && ((uintptr_t)X & 15) == 0,
             "dx_voc_post: bad shape (ncols >= N, ldy >= ncols, sxb %% 4 == 0, a 16-byte aligned X)");
  const dim3 grid(dx_cdiv(ncols, THREADS), B);
  if (C == 32)
    hipLaunchKernelGGL((voc_post_kernel<false, 32>), grid, dim3(THREADS), 0, (hipStream_t)stream, X, sxb, W, bias, Y, ldy, frames, scale, N,
                       ncols, WinArgs{});
  else
    hipLaunchKernelGGL((voc_post_kernel<false, 16>), grid, dim3(THREADS), 0, (hipStream_t)stream, X, sxb, W, bias, Y, ldy, frames, scale, N,
                       ncols, WinArgs{});
  DX_LAUNCH_CHECK("dx_voc_post");
  return DX_OK;
}

int dx_voc_post(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                int B, int N, int ncols, void* stream) {
  return dx_voc_post_c(X, sxb, W, bias, Y, ldy, frames, scale, B, N, ncols, 32, stream);
}

int dx_voc_post_c_win(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                      int B, int N, int ncols, int C, const int* cursor, int step, int lag, int mx, int my, void* stream) {
  DX_REQUIRE(X && W && bias && Y && frames, "dx_voc_post_win: null pointer");
  DX_REQUIRE(C == 16 || C == 32, "dx_voc_post_win: bad channel count (C in {16, 32})");
  DX_REQUIRE(voc_win_ok(cursor, step, lag, mx, my, 0) && my == 0, "dx_voc_post_win: bad window (cursor, step > 0, lag >= 0, mx 0 or 2^k - 1, my 0: the chunk buffer is not a ring)");
  DX_REQUIRE(B > 0 && N > 0 && scale > 0 && ncols >= step + lag && ldy >= ncols && sxb % 4 == 0 && ((uintptr_t)X & 15) == 0 &&
                 (mx ? (long)(mx + 1) : (long)N) * C <= sxb,
             "dx_voc_post_win: bad shape (ncols >= step + lag, ldy >= ncols, sxb %% 4 == 0 and holding X's ring, a 16-byte aligned X)");
  const WinArgs w = voc_win(cursor, step, lag, mx, 0, 0);
  const dim3 grid(dx_cdiv(step + lag, THREADS), B);
  if (C == 32)
    hipLaunchKernelGGL((voc_post_kernel<true, 32>), grid, dim3(THREADS), 0, (hipStream_t)stream, X, sxb, W, bias, Y, ldy, frames, scale, N,
                       ncols, w);
  else
    hipLaunchKernelGGL((voc_post_kernel<true, 16>), grid, dim3(THREADS), 0, (hipStream_t)stream, X, sxb, W, bias, Y, ldy, frames, scale, N,
                       ncols, w);
  DX_LAUNCH_CHECK("dx_voc_post_win");
  return DX_OK;
}

int dx_voc_post_win(const float* X, long sxb, const float* W, const float* bias, float* Y, int ldy, const int* frames, int scale,
                    int B, int N, int ncols, const int* cursor, int step, int lag, int mx, int my, void* stream) {
  return dx_voc_post_c_win(X, sxb, W, bias, Y, ldy, frames, scale, B, N, ncols, 32, cursor, step, lag, mx, my, stream);
}

int dx_voc_stream_advance(int* cursor, void* stream) {
  DX_REQUIRE(cursor, "dx_voc_stream_advance: null pointer");
  hipLaunchKernelGGL(voc_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, cursor);
  DX_LAUNCH_CHECK("dx_voc_stream_advance");
  return DX_OK;
}

}  // extern "C"
