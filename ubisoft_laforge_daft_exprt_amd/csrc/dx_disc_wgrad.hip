// HiFi-GAN discriminators, the discriminator step: the gradient of loss_disc with respect to the FOLDED (weight, bias)
// pair of every layer, over all 2B rows (real rows first).  The data gradient between layers is dx_disc_conv_dgrad, unchanged; this
// file holds the rest.  Buffers are the forward's: fp32, channels-last, rows addressed by (batch stride, column stride, position stride).
//
//   dx_disc_wgrad        G[co][ci_g][t] = sum_rows sum_m A[row][m s - pad + t][ci] dZ[row][m][co] (co in ci's group), dbias[co] = sum dZ,
//                        on v_mfma_f32_16x16x4_f32 with the POSITION as the MFMA k.  The k axis is the flattened (row, m) sequence, cut
//                        into tiles of KT (64) consecutive entries: a tile of a deep period layer (1 to 51 positions per row) holds
//                        several rows, none padded.  A workgroup owns <= 64 output channels x <= 64 input channels of one group and a
//                        GROUP of taps (all of them where the accumulators fit): it stages the dZ tile and ONE window of A with its halo
//                        -- per row segment (positions - 1) s + taps-in-group slots, 63 s + taps for a one-row tile -- and runs every tap
//                        of its group against them, accumulators in registers.  A "unit" is (tap, 16 output channels); wave w owns units
//                        w, w + 4, ...: the four waves split the taps and read the one staged window.  Only tap groups that do not fit
//                        the registers go to the grid.
//   dx_disc_post_wgrad   the score seed dS = w (2 / cnt) (S - [real row]), conv_post's dW, db (db summed in double) and the
//                        pre-activation gradient of the last conv layer.
//   dx_disc_first_wgrad  the Cin = 1 first layer's dW, db, read through the period view with the reflect tail applied while reading.
//
// Determinism.  No atomics.  Each k axis is cut into S runs of consecutive tiles (entries), S a function of the shape alone; run s adds
// its tiles in order and writes its partial sums to the caller's workspace; a second launch adds the S partials in order and writes
// the gradient in the parameter's own layout.  Two calls give the same bits.  No kernel here uses scratch.
#include "dx_common.h"

namespace {

constexpr float DW_SLOPE = 0.1f;
constexpr int THREADS = 256;
constexpr int WG_TARGET = 1024;          // the k split aims at this many workgroups
constexpr int S_CAP = 64;                // runs of the k axis, at most
constexpr long WS_CAP = 1L << 24;        // floats of partial G, at most (64 MB): the 21 MB gradient of a 1024 x 1024 x 5 layer gets S <= 3
constexpr int LDS_CAP = 64 * 1024;
constexpr int BLOCKS_PER_WAVE = 28;      // 16 x 16 accumulator blocks a wave keeps (112 registers)
constexpr int POST_TAPS = 8;             // conv_post: taps, at most
constexpr int FIRST_TAPS = 16;           // first layer: taps, at most

__host__ __device__ __forceinline__ long wg_row_offset(int row, int rdiv, long sb, long sr) {
  const int rb = row / rdiv, rc = row - rb * rdiv;
  return rb * sb + rc * sr;
}

struct WgPlan {
  int Cin_g, Cout_g, Nout, cot, cit, ncob, nci, ncit, ntg, TG, upw, KT, ldz, ldx, slots, tiles, S, per, K;
  long nG;
  size_t smem;
};

// The tiling and the split: a fixed function of the shape.
bool wg_plan(int rows, int N, int Cin, int Cout, int groups, int taps, int stride, int pad, WgPlan& p) {
  if (rows <= 0 || N <= 0 || Cin <= 0 || Cout <= 0 || groups <= 0 || Cin % groups != 0 || Cout % groups != 0) return false;
  if (taps < 1 || taps > 41 || stride < 1 || stride > 4 || pad < 0 || pad > 20 || N + 2 * pad < taps) return false;
  p.Cin_g = Cin / groups;
  p.Cout_g = Cout / groups;
  if (p.Cout_g != 16 && p.Cout_g != 32 && p.Cout_g % 64 != 0) return false;
  if (p.Cin_g != 8 && p.Cin_g != 16 && p.Cin_g != 32 && p.Cin_g % 64 != 0) return false;
  p.cot = p.Cout_g < 64 ? p.Cout_g : 64;
  p.cit = p.Cin_g == 8 ? 16 : (p.Cin_g < 64 ? p.Cin_g : 64);
  p.ncob = p.cot / 16;
  p.nci = p.cit / 16;
  p.ncit = p.Cin_g == 8 ? 1 : p.Cin_g / p.cit;
  p.Nout = (N + 2 * pad - taps) / stride + 1;
  const long K = (long)rows * p.Nout;
  if (K > 0x7fffffffL / 4) return false;
  p.K = (int)K;
  p.nG = (long)Cout * p.Cin_g * taps;
  const int tg_max = 4 * (BLOCKS_PER_WAVE / p.nci) / p.ncob;
  p.ntg = dx_cdiv(taps, tg_max);
  p.TG = dx_cdiv(taps, p.ntg);
  p.ntg = dx_cdiv(taps, p.TG);
  p.upw = dx_cdiv(p.TG * p.ncob, 4);
  p.ldz = p.cot % 32 == 16 ? p.cot : p.cot + 16;       // == 16 (mod 32): the four k rows of an operand read fall on disjoint banks
  p.ldx = p.cit + 4;
  for (int q = 0; q < 32; q += 4)                      // stride x ldx == 16 (mod 32): the same for window slots `stride` apart
    if ((stride * (p.cit + q)) % 32 == 16) { p.ldx = p.cit + q; break; }
  const int step = p.TG > stride ? p.TG : stride;
  p.KT = 0;
  for (int kt = 64; kt >= 4; kt >>= 1) {               // the largest tile whose worst-case window (every row segment with its halo) fits
    const int nseg = (kt - 2) / p.Nout + 2 < kt ? (kt - 2) / p.Nout + 2 : kt;
    const long slots = (long)(kt - 1) * stride + (long)nseg * step;
    const size_t smem = ((size_t)kt * p.ldz + (size_t)(slots + p.TG) * p.ldx + kt) * 4;
    if (smem <= (size_t)LDS_CAP) { p.KT = kt; p.slots = (int)slots; p.smem = smem; break; }
  }
  if (!p.KT) return false;
  p.tiles = dx_cdiv(p.K, p.KT);
  const long blocks = (long)(Cout / p.cot) * p.ncit * p.ntg;
  if (Cout / p.cot > 65535 || (long)p.ncit * p.ntg > 65535) return false;
  long S = WG_TARGET / blocks > 1 ? WG_TARGET / blocks : 1;
  if (S > S_CAP) S = S_CAP;
  if (S > WS_CAP / p.nG) S = WS_CAP / p.nG > 1 ? WS_CAP / p.nG : 1;
  if (S > p.tiles) S = p.tiles;
  p.per = dx_cdiv(p.tiles, (int)S);
  p.S = dx_cdiv(p.tiles, p.per);
  return true;
}

struct WgArgs {
  const float* A; long sxb, sxr, sxn;
  const float* dZ; long szb, szr, szn;
  float* P; float* Pb;
  int rows, rdiv, N, Nout, Cin_g, Cout_g, Cout, taps, stride, pad, cot, cit, ncob, ncit, TG, KT, ldz, ldx, slots, tiles, per, K;
  long nG;
};

// Window slot of k entry (row, m) of a tile that starts at (row0, m0): row segments follow each other, each with its own halo.
__device__ __forceinline__ int wg_slot(int row, int m, int row0, int m0, int len0, int L, int stride) {
  return row == row0 ? (m - m0) * stride : len0 + (row - row0 - 1) * L + m * stride;
}

// UPW: units (tap, 16 output channels) per wave; NCI: 16-wide input-channel blocks of the workgroup's tile
template <int UPW, int NCI>
__global__ void __launch_bounds__(THREADS) disc_wgrad_kernel(WgArgs p) {
  extern __shared__ __attribute__((aligned(16))) float wg_smem[];
  float* Zs = wg_smem;
  float* Xs = Zs + p.KT * p.ldz;
  int* Off = reinterpret_cast<int*>(Xs + (p.slots + p.TG) * p.ldx);
  const int s = blockIdx.x, co0 = blockIdx.y * p.cot, grp = co0 / p.Cout_g;
  const int tg = blockIdx.z / p.ncit, cib = blockIdx.z - tg * p.ncit;
  const int t0 = tg * p.TG, tgc = min(p.TG, p.taps - t0);
  const int cig0 = cib * p.cit, creal = min(p.cit, p.Cin_g - cig0), ci0 = grp * p.Cin_g + cig0;
  const int NU = tgc * p.ncob;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const bool bias_block = blockIdx.z == 0;
  int zc[UPW], xr[UPW];
#pragma unroll
  for (int j = 0; j < UPW; ++j) {
    const int u = w + 4 * j, t = u / p.ncob, cob = u - t * p.ncob;
    zc[j] = cob * 16 + r;
    xr[j] = t * p.ldx + r;
  }
  f32x4 acc[UPW][NCI] = {};
  float bsum = 0.f;
  for (int e = tid; e < p.TG * p.ldx; e += THREADS) Xs[p.slots * p.ldx + e] = 0.f;     // where the k entries past the end point
  const int L = (p.Nout - 1) * p.stride + p.TG;
  const int q1 = min((s + 1) * p.per, p.tiles);
  for (int q = s * p.per; q < q1; ++q) {
    const int f0 = q * p.KT, row0 = f0 / p.Nout, m0 = f0 - row0 * p.Nout;
    const int len0 = (p.Nout - 1 - m0) * p.stride + p.TG;
    const int fl = min(f0 + p.KT, p.K) - 1, rowl = fl / p.Nout;
    const int nslots = wg_slot(rowl, fl - rowl * p.Nout, row0, m0, len0, L, p.stride) + p.TG;
    __syncthreads();
    if (tid < p.KT) {
      const int f = f0 + tid;
      int off = p.slots;
      if (f < p.K) {
        const int row = f / p.Nout;
        off = wg_slot(row, f - row * p.Nout, row0, m0, len0, L, p.stride);
      }
      Off[tid] = off * p.ldx;
    }
    const int qz = p.cot >> 2;
    for (int e = tid; e < p.KT * qz; e += THREADS) {
      const int rr = e / qz, cc = (e - rr * qz) * 4, f = f0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f < p.K) {
        const int row = f / p.Nout, m = f - row * p.Nout;
        v = *reinterpret_cast<const float4*>(p.dZ + wg_row_offset(row, p.rdiv, p.szb, p.szr) + (long)m * p.szn + co0 + cc);
      }
      *reinterpret_cast<float4*>(Zs + rr * p.ldz + cc) = v;
    }
    const int qx = p.cit >> 2;
    for (int e = tid; e < nslots * qx; e += THREADS) {
      const int wv = e / qx, cc = (e - wv * qx) * 4;
      int row = row0, pos = m0 * p.stride - p.pad + t0 + wv;
      if (wv >= len0) {
        const int w2 = wv - len0, i = w2 / L;
        row = row0 + 1 + i;
        pos = w2 - i * L - p.pad + t0;
      }
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (cc < creal && row < p.rows && pos >= 0 && pos < p.N)
        v = *reinterpret_cast<const float4*>(p.A + wg_row_offset(row, p.rdiv, p.sxb, p.sxr) + (long)pos * p.sxn + ci0 + cc);
      *reinterpret_cast<float4*>(Xs + wv * p.ldx + cc) = v;
    }
    __syncthreads();
    if (bias_block && tid < p.cot) {
      for (int rr = 0; rr < p.KT; ++rr) bsum += Zs[rr * p.ldz + tid];
    }
    for (int k0 = 0; k0 < p.KT; k0 += 4) {
      const float* zrow = Zs + (k0 + g) * p.ldz;
      const float* xrow = Xs + Off[k0 + g];
#pragma unroll
      for (int j = 0; j < UPW; ++j) {
        if (w + 4 * j < NU) {
          const float a = zrow[zc[j]];
#pragma unroll
          for (int i = 0; i < NCI; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xrow[xr[j] + i * 16], acc[j][i], 0, 0, 0);
        }
      }
    }
  }
  float* P = p.P + (long)s * p.nG;
#pragma unroll
  for (int j = 0; j < UPW; ++j) {
    const int u = w + 4 * j;
    if (u < NU) {
      const int tt = u / p.ncob, cob = u - tt * p.ncob;
#pragma unroll
      for (int i = 0; i < NCI; ++i) {
        const int ci = cig0 + i * 16 + r;
        if (ci < p.Cin_g) {
#pragma unroll
          for (int e = 0; e < 4; ++e) P[((long)(co0 + cob * 16 + 4 * g + e) * p.Cin_g + ci) * p.taps + t0 + tt] = acc[j][i][e];
        }
      }
    }
  }
  if (bias_block && tid < p.cot) p.Pb[(long)s * p.Cout + co0 + tid] = bsum;
}

// out[e] = sum over the S partials, in order; the nG weight elements, then the nB bias elements
__global__ void disc_wgrad_reduce_kernel(const float* P, const float* Pb, float* G, float* dbias, int S, long nG, int nB) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nG) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += P[(long)s * nG + e];
    G[e] = a;
  } else if (e < nG + nB) {
    const int c = (int)(e - nG);
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += Pb[(long)s * nB + c];
    dbias[c] = a;
  }
}

template <int UPW, int NCI>
int launch_wgrad(const WgArgs& a, const WgPlan& pl, hipStream_t s) {
  hipLaunchKernelGGL((disc_wgrad_kernel<UPW, NCI>), dim3(pl.S, a.Cout / pl.cot, pl.ncit * pl.ntg), dim3(THREADS), pl.smem, s, a);
  DX_LAUNCH_CHECK("dx_disc_wgrad");
  return DX_OK;
}

int dispatch_wgrad(const WgArgs& a, const WgPlan& pl, hipStream_t s) {
  if (pl.nci == 1) {
    if (pl.upw <= 11) return launch_wgrad<11, 1>(a, pl, s);
    if (pl.upw <= 21) return launch_wgrad<21, 1>(a, pl, s);
    return launch_wgrad<28, 1>(a, pl, s);
  }
  if (pl.nci == 2) {
    if (pl.upw <= 5) return launch_wgrad<5, 2>(a, pl, s);
    if (pl.upw <= 11) return launch_wgrad<11, 2>(a, pl, s);
    return launch_wgrad<14, 2>(a, pl, s);
  }
  if (pl.upw <= 5) return launch_wgrad<5, 4>(a, pl, s);
  return launch_wgrad<7, 4>(a, pl, s);
}

// ---- conv_post ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float post_seed(const float* S, long off, int row, int half_rows, float wsc) {
  return wsc * (row < half_rows ? S[off] - 1.f : S[off]);
}

// dZ[row][n][c] = slope(A[row][n][c]) sum_t dS[row][n + pad - t] W[c][t]: one thread per position and 4 channels
__global__ void __launch_bounds__(THREADS) disc_post_dz_kernel(const float* S, long ssb, long ssr, long ssn, const float* W, const float* A,
                                                               float* dZ, long sxb, long sxr, long sxn, const float* gw, float s_scale,
                                                               int half_rows, int rdiv, int N, int C, int taps, long total) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= total) return;
  const int c4 = C >> 2;
  const int c = (int)(e % c4) * 4;
  const long pos = e / c4;
  const int n = (int)(pos % N), row = (int)(pos / N), pad = (taps - 1) / 2;
  const long so = wg_row_offset(row, rdiv, ssb, ssr);
  const float wsc = gw[0] * s_scale;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int t = 0; t < taps; ++t) {
    const int m = n + pad - t;
    if (m < 0 || m >= N) continue;
    const float ds = post_seed(S, so + (long)m * ssn, row, half_rows, wsc);
    a0 = __builtin_fmaf(ds, W[(long)(c + 0) * taps + t], a0);
    a1 = __builtin_fmaf(ds, W[(long)(c + 1) * taps + t], a1);
    a2 = __builtin_fmaf(ds, W[(long)(c + 2) * taps + t], a2);
    a3 = __builtin_fmaf(ds, W[(long)(c + 3) * taps + t], a3);
  }
  const long off = wg_row_offset(row, rdiv, sxb, sxr) + (long)n * sxn + c;
  const float4 av = *reinterpret_cast<const float4*>(A + off);
  *reinterpret_cast<float4*>(dZ + off) = make_float4(a0 * (av.x > 0.f ? 1.f : DW_SLOPE), a1 * (av.y > 0.f ? 1.f : DW_SLOPE),
                                                     a2 * (av.z > 0.f ? 1.f : DW_SLOPE), a3 * (av.w > 0.f ? 1.f : DW_SLOPE));
}

// Run blockIdx.x of the flattened (row, m) axis, channel blockIdx.y * THREADS + tid: P[s][c][t] = sum dS[row][m] A[row][m - pad + t][c];
// the run's sum of dS in double.
__global__ void __launch_bounds__(THREADS) disc_post_wgrad_kernel(const float* S, long ssb, long ssr, long ssn, const float* A, long sxb,
                                                                  long sxr, long sxn, const float* gw, float s_scale, int half_rows, int rdiv,
                                                                  int N, int C, int taps, int K, int per, float* P, double* Pd) {
  const int s = blockIdx.x, c = blockIdx.y * THREADS + threadIdx.x, pad = (taps - 1) / 2;
  const float wsc = gw[0] * s_scale;
  float acc[POST_TAPS];
#pragma unroll
  for (int t = 0; t < POST_TAPS; ++t) acc[t] = 0.f;
  double dsum = 0.0;
  const int f1 = min((s + 1) * per, K);
  for (int f = s * per; f < f1; ++f) {
    const int row = f / N, m = f - row * N;
    const float ds = post_seed(S, wg_row_offset(row, rdiv, ssb, ssr) + (long)m * ssn, row, half_rows, wsc);
    dsum += (double)ds;
    if (c < C) {
      const float* a = A + wg_row_offset(row, rdiv, sxb, sxr) + c;
#pragma unroll
      for (int t = 0; t < POST_TAPS; ++t) {
        const int pos = m - pad + t;
        if (t < taps && pos >= 0 && pos < N) acc[t] = __builtin_fmaf(ds, a[(long)pos * sxn], acc[t]);
      }
    }
  }
  if (c < C) {
#pragma unroll
    for (int t = 0; t < POST_TAPS; ++t)
      if (t < taps) P[((long)s * C + c) * taps + t] = acc[t];
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) Pd[s] = dsum;
}

__global__ void disc_post_reduce_kernel(const float* P, const double* Pd, float* dW, float* db, int S, long nG) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nG) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += P[(long)s * nG + e];
    dW[e] = a;
  } else if (e == nG) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += Pd[s];
    db[0] = (float)a;
  }
}

int post_runs(long K) {
  const long s = K / 8;
  return (int)(s < 1 ? 1 : (s > 128 ? 128 : s));
}

// ---- the first layer ------------------------------------------------------------------------------------------------------------
// Thread (sub, co) of run blockIdx.x takes the run's entries (b, m, column) sub, sub + nsub, ... in order: its taps' sums and its bias sum
// go to partial s * nsub + sub.
__global__ void __launch_bounds__(THREADS) disc_first_wgrad_kernel(const float* x, long sxb, int T, const float* dZ, float* P, float* Pb,
                                                                   int p, int H, int Hout, int Cout, int taps, int stride, int pad, int K,
                                                                   int per) {
  const int nsub = THREADS / Cout, sub = threadIdx.x / Cout, co = threadIdx.x - sub * Cout;
  if (sub >= nsub) return;
  float acc[FIRST_TAPS];
#pragma unroll
  for (int t = 0; t < FIRST_TAPS; ++t) acc[t] = 0.f;
  float bsum = 0.f;
  const int f1 = min((int)(blockIdx.x + 1) * per, K);
  for (int f = blockIdx.x * per + sub; f < f1; f += nsub) {
    const int wc = f % p, q = f / p, m = q % Hout, b = q / Hout;
    const float dz = dZ[(long)f * Cout + co];
    const float* xr = x + (long)b * sxb;
    bsum += dz;
#pragma unroll
    for (int t = 0; t < FIRST_TAPS; ++t) {          // every load is unconditional (a tap outside the view reads row 0 and adds zero)
      const int h = m * stride - pad + t;
      const bool in = t < taps && h >= 0 && h < H;
      long i = (long)(in ? h : 0) * p + wc;
      if (i >= T) i = 2L * (T - 1) - i;
      acc[t] = __builtin_fmaf(in ? xr[i] : 0.f, dz, acc[t]);
    }
  }
  const long part = (long)blockIdx.x * nsub + sub;
#pragma unroll
  for (int t = 0; t < FIRST_TAPS; ++t)
    if (t < taps) P[(part * Cout + co) * taps + t] = acc[t];
  Pb[part * Cout + co] = bsum;
}

// The first layer has up to 2048 partials of only Cout (taps + 1) outputs: one wave per output; lane l adds partials l, l + 64, ... in
// order, then a fixed butterfly joins the lanes.  P is [parts][nG], Pb [parts][nB].
__global__ void __launch_bounds__(THREADS) disc_first_reduce_kernel(const float* P, const float* Pb, float* G, float* dbias, int parts, int nG,
                                                                    int nB) {
  const int e = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (e >= nG + nB) return;
  const float* src = e < nG ? P + e : Pb + (e - nG);
  const int ld = e < nG ? nG : nB;
  float a = 0.f;
  for (int s = lane; s < parts; s += 64) a += src[(long)s * ld];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
  if (lane == 0) (e < nG ? G[e] : dbias[e - nG]) = a;
}

int first_runs(long K, int nsub) {
  const long s = K / (16L * nsub);
  return (int)(s < 1 ? 1 : (s > 1024 ? 1024 : s));
}

}  // namespace

extern "C" {

int dx_disc_wgrad_size(int rows, int N, int Cin, int Cout, int groups, int taps, int stride, int pad, long* bytes, int* splits) {
  DX_REQUIRE(bytes, "dx_disc_wgrad_size: null output");
  WgPlan pl;
  DX_REQUIRE(wg_plan(rows, N, Cin, Cout, groups, taps, stride, pad, pl),
             "dx_disc_wgrad_size: bad shape (channels per group: in 8, 16, 32 or a multiple of 64, out 16, 32 or a multiple of 64; "
             "taps <= 41, stride <= 4, pad <= 20, N + 2 pad >= taps)");
  *bytes = (long)pl.S * (pl.nG + Cout) * 4;
  if (splits) *splits = pl.S;
  return DX_OK;
}

int dx_disc_wgrad(const float* A, long sxb, long sxr, long sxn, const float* dZ, long szb, long szr, long szn, float* G, float* dbias,
                  void* workspace, long workspace_bytes, int rows, int rdiv, int N, int Cin, int Cout, int groups, int taps, int stride,
                  int pad, void* stream) {
  DX_REQUIRE(A && dZ && G && dbias && workspace, "dx_disc_wgrad: null pointer");
  DX_REQUIRE(rdiv > 0, "dx_disc_wgrad: non-positive rdiv");
  WgPlan pl;
  DX_REQUIRE(wg_plan(rows, N, Cin, Cout, groups, taps, stride, pad, pl),
             "dx_disc_wgrad: bad shape (channels per group: in 8, 16, 32 or a multiple of 64, out 16, 32 or a multiple of 64; "
             "taps <= 41, stride <= 4, pad <= 20, N + 2 pad >= taps)");
  DX_REQUIRE(sxn % 4 == 0 && sxr % 4 == 0 && sxb % 4 == 0 && dx_aligned16(A) && szn % 4 == 0 && szr % 4 == 0 && szb % 4 == 0 && dx_aligned16(dZ),
             "dx_disc_wgrad: A and dZ need strides %% 4 == 0 and 16-byte aligned pointers");
  DX_REQUIRE(workspace_bytes >= (long)pl.S * (pl.nG + Cout) * 4 && dx_aligned16(workspace),
             "dx_disc_wgrad: workspace smaller than dx_disc_wgrad_size reports");
  WgArgs a;
  a.A = A; a.sxb = sxb; a.sxr = sxr; a.sxn = sxn;
  a.dZ = dZ; a.szb = szb; a.szr = szr; a.szn = szn;
  a.P = reinterpret_cast<float*>(workspace);
  a.Pb = a.P + (long)pl.S * pl.nG;
  a.rows = rows; a.rdiv = rdiv; a.N = N; a.Nout = pl.Nout; a.Cin_g = pl.Cin_g; a.Cout_g = pl.Cout_g; a.Cout = Cout; a.taps = taps;
  a.stride = stride; a.pad = pad; a.cot = pl.cot; a.cit = pl.cit; a.ncob = pl.ncob; a.ncit = pl.ncit; a.TG = pl.TG; a.KT = pl.KT;
  a.ldz = pl.ldz; a.ldx = pl.ldx; a.slots = pl.slots; a.tiles = pl.tiles; a.per = pl.per; a.K = pl.K; a.nG = pl.nG;
  hipStream_t s = (hipStream_t)stream;
  const int rc = dispatch_wgrad(a, pl, s);
  if (rc != DX_OK) return rc;
  hipLaunchKernelGGL(disc_wgrad_reduce_kernel, dim3((unsigned)((pl.nG + Cout + 255) / 256)), dim3(256), 0, s, a.P, a.Pb, G, dbias, pl.S,
                     pl.nG, Cout);
  DX_LAUNCH_CHECK("dx_disc_wgrad (reduce)");
  return DX_OK;
}

int dx_disc_post_wgrad_size(int rows, int N, int C, int taps, long* bytes) {
  DX_REQUIRE(bytes, "dx_disc_post_wgrad_size: null output");
  DX_REQUIRE(rows > 0 && N > 0 && C > 0 && C % 4 == 0 && taps > 0 && taps <= POST_TAPS && taps % 2 == 1 && (long)rows * N <= 0x3fffffffL,
             "dx_disc_post_wgrad_size: bad shape (positive sizes, C %% 4 == 0, odd taps <= 8)");
  const int S = post_runs((long)rows * N);
  *bytes = (long)S * 8 + (long)S * C * taps * 4;
  return DX_OK;
}

int dx_disc_post_wgrad(const float* S, long ssb, long ssr, long ssn, const float* W, const float* A, float* dZ, long sxb, long sxr, long sxn,
                       const float* gw, float s_scale, float* dW, float* db, void* workspace, long workspace_bytes, int rows,
                       int half_rows, int rdiv, int N, int C, int taps, void* stream) {
  DX_REQUIRE(S && W && A && dZ && gw && dW && db && workspace, "dx_disc_post_wgrad: null pointer");
  DX_REQUIRE(rows > 0 && rdiv > 0 && N > 0 && C > 0 && C % 4 == 0 && taps > 0 && taps <= POST_TAPS && taps % 2 == 1 &&
                 (long)rows * N <= 0x3fffffffL && half_rows >= 0 && half_rows <= rows,
             "dx_disc_post_wgrad: bad shape (positive sizes, C %% 4 == 0, odd taps <= 8, 0 <= half_rows <= rows)");
  DX_REQUIRE(sxn % 4 == 0 && sxr % 4 == 0 && sxb % 4 == 0 && dx_aligned16(dZ) && dx_aligned16(A),
             "dx_disc_post_wgrad: the maps need strides %% 4 == 0 and 16-byte aligned pointers");
  DX_REQUIRE((const void*)A != (const void*)dZ, "dx_disc_post_wgrad: dZ must not alias A (the weight gradient reads A after dZ is written)");
  const int K = rows * N, runs = post_runs(K), per = dx_cdiv(K, runs);
  const long nG = (long)C * taps;
  DX_REQUIRE(workspace_bytes >= (long)runs * 8 + (long)runs * nG * 4 && ((uintptr_t)workspace & 7) == 0,
             "dx_disc_post_wgrad: workspace smaller than dx_disc_post_wgrad_size reports");
  double* Pd = reinterpret_cast<double*>(workspace);
  float* P = reinterpret_cast<float*>(Pd + runs);
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)rows * N * (C / 4);
  DX_REQUIRE((total + THREADS - 1) / THREADS <= 0x7fffffffL, "dx_disc_post_wgrad: too many outputs for one launch");
  hipLaunchKernelGGL(disc_post_dz_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, S, ssb, ssr, ssn, W, A, dZ,
                     sxb, sxr, sxn, gw, s_scale, half_rows, rdiv, N, C, taps, total);
  DX_LAUNCH_CHECK("dx_disc_post_wgrad (dZ)");
  hipLaunchKernelGGL(disc_post_wgrad_kernel, dim3(runs, dx_cdiv(C, THREADS)), dim3(THREADS), 0, s, S, ssb, ssr, ssn, A, sxb, sxr, sxn, gw,
                     s_scale, half_rows, rdiv, N, C, taps, K, per, P, Pd);
  DX_LAUNCH_CHECK("dx_disc_post_wgrad");
  hipLaunchKernelGGL(disc_post_reduce_kernel, dim3((unsigned)((nG + 1 + 255) / 256)), dim3(256), 0, s, P, Pd, dW, db, runs, nG);
  DX_LAUNCH_CHECK("dx_disc_post_wgrad (reduce)");
  return DX_OK;
}

int dx_disc_first_wgrad_size(int R, int T, int p, int Cout, int taps, int stride, int pad, long* bytes) {
  DX_REQUIRE(bytes, "dx_disc_first_wgrad_size: null output");
  DX_REQUIRE(R > 0 && T > 0 && p > 0 && Cout > 0 && Cout <= THREADS && THREADS % Cout == 0 && taps > 0 && taps <= FIRST_TAPS && stride > 0 &&
                 pad >= 0 && dx_cdiv(T, p) + 2 * pad >= taps,
             "dx_disc_first_wgrad_size: bad shape (positive sizes, Cout a divisor of 256, taps <= 16, H + 2 pad >= taps)");
  const int Hout = (dx_cdiv(T, p) + 2 * pad - taps) / stride + 1;
  const long K = (long)R * Hout * p;
  DX_REQUIRE(K <= 0x3fffffffL, "dx_disc_first_wgrad_size: too many positions");
  const int nsub = THREADS / Cout;
  *bytes = (long)first_runs(K, nsub) * nsub * Cout * (taps + 1) * 4;
  return DX_OK;
}

int dx_disc_first_wgrad(const float* x, long sxb, int T, const float* dZ, float* dW, float* db, void* workspace, long workspace_bytes, int R,
                        int p, int Cout, int taps, int stride, int pad, void* stream) {
  DX_REQUIRE(x && dZ && dW && db && workspace, "dx_disc_first_wgrad: null pointer");
  DX_REQUIRE(R > 0 && T > 0 && p > 0 && Cout > 0 && Cout <= THREADS && THREADS % Cout == 0 && taps > 0 && taps <= FIRST_TAPS && stride > 0 &&
                 pad >= 0 && sxb >= T && dx_cdiv(T, p) + 2 * pad >= taps,
             "dx_disc_first_wgrad: bad shape (positive sizes, Cout a divisor of 256, taps <= 16, sxb >= T, H + 2 pad >= taps)");
  DX_REQUIRE(T % p == 0 || p - T % p < T, "dx_disc_first_wgrad: the reflect padding (p - T %% p samples) must be shorter than the signal");
  const int H = dx_cdiv(T, p), Hout = (H + 2 * pad - taps) / stride + 1;
  const long K = (long)R * Hout * p;
  DX_REQUIRE(K <= 0x3fffffffL, "dx_disc_first_wgrad: too many positions");
  const int nsub = THREADS / Cout, runs = first_runs(K, nsub), per = dx_cdiv((int)K, runs), parts = runs * nsub;
  const long nG = (long)Cout * taps;
  DX_REQUIRE(workspace_bytes >= (long)parts * (nG + Cout) * 4 && ((uintptr_t)workspace & 3) == 0,
             "dx_disc_first_wgrad: workspace smaller than dx_disc_first_wgrad_size reports");
  float* P = reinterpret_cast<float*>(workspace);
  float* Pb = P + (long)parts * nG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(disc_first_wgrad_kernel, dim3(runs), dim3(THREADS), 0, s, x, sxb, T, dZ, P, Pb, p, H, Hout, Cout, taps, stride, pad, (int)K,
                     per);
  DX_LAUNCH_CHECK("dx_disc_first_wgrad");
  hipLaunchKernelGGL(disc_first_reduce_kernel, dim3((unsigned)dx_cdiv((int)nG + Cout, THREADS / 64)), dim3(THREADS), 0, s, P, Pb, dW, db, parts,
                     (int)nG, Cout);
  DX_LAUNCH_CHECK("dx_disc_first_wgrad (reduce)");
  return DX_OK;
}

}  // extern "C"
