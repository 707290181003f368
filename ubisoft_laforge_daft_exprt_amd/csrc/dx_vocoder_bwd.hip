// HiFi-GAN generator training, f32 operand mode: the kernels the backward adds to csrc/dx_vocoder.hip.  Every DATA gradient of the
// generator runs through dx_voc_conv with a pack built on the host (vocoder_train.py: a dilated conv's flipped, transposed weight; a
// transposed conv's three-tap view); this file holds the rest:
//
//   dx_voc_wgrad      G[co][ci][t] = sum_b sum_n act(X[b][n - pad + t dil][ci]) dY[b][n][co], dbias[co] = sum dY, on v_mfma_f32_16x16x4_f32
//                     with the POSITION n as the MFMA k.  A tile is 64 positions of one batch row: dY (64 x <= 64 output channels) and the
//                     tap's own 64 rows of X (<= 64 input channels, act applied while staging) in LDS, channels last, rows padded so that
//                     the four rows one operand read touches fall on disjoint banks.  The tap is on the grid (grid.z), so a workgroup
//                     keeps 16 accumulator registers per lane whatever the kernel width; X is then read once per tap, from L2.
//                     A ConvTranspose1d(k = 2u, stride u, padding u / 2) is the three-tap case on the view dY (N u, Cout) -> (N, u Cout),
//                     one phase r (a channel offset r Cout) at a time: grid.z = 3 u, of which the 2 u (phase, tap) pairs that name a
//                     kernel index do any work.
//   dx_voc_act_bwd    dX = acc( scale lrelu'(Xsaved) U (+ R) ), float4.
//   dx_voc_post_bwd   conv_post with y = clip(tanh z): dz = dy (1 - y^2), dX = lrelu'(x) convT(dz), dw, db.
//
// Determinism.  No atomics.  The position axis (B x ceil(N / 64) tiles, row-major) is cut into S runs of equal length, S a function of
// the shape alone (voc_wgrad_plan); run s accumulates its tiles in order and writes its partial sums to a caller's workspace; a
// second launch adds the S partials in order and writes the weight gradient in the parameter's own layout.  Two calls give the same
// bits.  Rows at or past min(frames[b] scale, N) read as zero in both operands and are written as zero.
#include "dx_common.h"

namespace {

constexpr float BWD_SLOPE = 0.1f;
constexpr int WT = 64;            // positions per tile: 16 MFMA k steps
constexpr int WC = 64;            // channels per tile, either operand: 4 x 4 MFMA blocks, four per wave
constexpr int THREADS = 256;
constexpr int WGRAD_BLOCKS = 2048;     // the split aims at this many workgroups
constexpr int PT = 256;           // conv_post: samples per pass
constexpr int PPASS = 4;          //            passes per workgroup

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * BWD_SLOPE; }
__device__ __forceinline__ float dlrelu(float v) { return v > 0.f ? 1.f : BWD_SLOPE; }

// LDS row length of a tile of w channels (w % 16 == 0): == 16 (mod 32), so rows k and k + 1 of a ds_read_b32 operand read (lanes
// 0-15 and 16-31 of one 32-lane group) sit 16 banks apart
__host__ __device__ inline int tile_ld(int w) { return (w % 32 == 16) ? w : w + 16; }

struct WgradPlan {
  int tilesN, total, S, per, nco, nci, Z, nph;
  long g_elems, b_elems;
};

// The split: a fixed function of the shape.  total tiles in S runs of `per` consecutive tiles.
bool voc_wgrad_plan(int B, int N, int Cin, int Cout, int taps, int up, WgradPlan& p) {
  const long total = (long)B * dx_cdiv(N, WT);
  if (total <= 0 || total > 0x7fffffffL) return false;
  p.tilesN = dx_cdiv(N, WT);
  p.total = (int)total;
  p.nco = dx_cdiv(Cout, WC);
  p.nci = dx_cdiv(Cin, WC);
  p.nph = up > 1 ? up : 1;
  p.Z = p.nph * taps;
  const long blocks = (long)p.Z * p.nco * p.nci;
  const int want = (int)(WGRAD_BLOCKS / blocks > 1 ? WGRAD_BLOCKS / blocks : 1);
  p.S = p.total < want ? p.total : want;
  p.per = dx_cdiv(p.total, p.S);
  p.S = dx_cdiv(p.total, p.per);
  p.g_elems = (long)p.S * p.Z * Cout * Cin;
  p.b_elems = (long)p.S * p.nph * Cout;
  return p.S <= 65535;
}

struct WgradArgs {
  const float* X; long sxb, sxn, sxc;
  const float* dY; long dyb; int ldy, dyc;
  float* P; float* Pb;
  const int* frames; int scale;
  int N, Cin, Cout, taps, dil, pad, up, act, tilesN, total, per, nci, Z, nph;
};

__global__ void __launch_bounds__(THREADS) voc_wgrad_kernel(WgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) float wg_smem[];
  const int s = blockIdx.x, z = blockIdx.z;
  const int cot = blockIdx.y / p.nci, cit = blockIdx.y - cot * p.nci;
  const int co0 = cot * WC, ci0 = cit * WC;
  const int tco = min(WC, p.Cout - co0), tci = min(WC, p.Cin - ci0);
  int t = z, ph = 0;
  if (p.up > 1) {                  // tap t reads a[n - 1 + t]: kernel index (1 - t) up + ph + up / 2, in [0, 2 up) for these pairs only
    ph = z / 3;
    t = z - ph * 3;
    if ((t == 2 && ph < p.up / 2) || (t == 0 && ph >= p.up / 2)) return;
  }
  const bool bias_block = cit == 0 && t == (p.up > 1 ? 1 : 0);
  const int shift = t * p.dil - p.pad;
  const int lda = tile_ld(tco), ldb = tile_ld(tci);
  float* Ys = wg_smem;
  float* Xs = wg_smem + WT * tile_ld(WC);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
  const int nbc = tci / 16, nblk = (tco / 16) * nbc, per_w = (nblk + 3) / 4;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int q1 = min((s + 1) * p.per, p.total);
  for (int q = s * p.per; q < q1; ++q) {
    const int b = q / p.tilesN, n0 = (q - b * p.tilesN) * WT;
    const int len = min(p.frames[b] * p.scale, p.N);
    if (n0 >= len) continue;                                   // the whole tile of dY is zero (uniform over the workgroup)
    const float* dY = p.dY + (long)b * p.dyb + p.dyc + (long)ph * p.Cout + co0;
    const float* X = p.X + (long)b * p.sxb;
    __syncthreads();
    const int qa = tco >> 2;
    for (int e = tid; e < WT * qa; e += THREADS) {
      const int rr = e / qa, cc = (e - rr * qa) * 4, n = n0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < len) v = *reinterpret_cast<const float4*>(dY + (long)n * p.ldy + cc);
      *reinterpret_cast<float4*>(Ys + rr * lda + cc) = v;
    }
    if (p.sxc == 1 && p.sxn >= p.Cin) {                        // channels last: float4 along the channels
      const int qb = tci >> 2;
      for (int e = tid; e < WT * qb; e += THREADS) {
        const int rr = e / qb, cc = (e - rr * qb) * 4, n = n0 + rr + shift;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n >= 0 && n < len) {
          v = *reinterpret_cast<const float4*>(X + (long)n * p.sxn + ci0 + cc);
          if (p.act) { v.x = lrelu(v.x); v.y = lrelu(v.y); v.z = lrelu(v.z); v.w = lrelu(v.w); }
        }
        *reinterpret_cast<float4*>(Xs + rr * ldb + cc) = v;
      }
    } else {                                                   // any other layout (the (B, 80, T) mel): consecutive threads along n
      for (int e = tid; e < WT * tci; e += THREADS) {
        const int cc = e / WT, rr = e - cc * WT, n = n0 + rr + shift;
        float v = 0.f;
        if (n >= 0 && n < len) {
          v = X[(long)n * p.sxn + (long)(ci0 + cc) * p.sxc];
          if (p.act) v = lrelu(v);
        }
        Xs[rr * ldb + cc] = v;
      }
    }
    __syncthreads();
    if (bias_block && tid < tco) {
      for (int rr = 0; rr < WT; ++rr) bsum += Ys[rr * lda + tid];
    }
    for (int k0 = 0; k0 < WT; k0 += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int id = w * per_w + j;
        if (j < per_w && id < nblk) {
          const int cob = id / nbc, cib = id - cob * nbc;
          const float a = Ys[(k0 + g) * lda + cob * 16 + r];
          const float x = Xs[(k0 + g) * ldb + cib * 16 + r];
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, x, acc[j], 0, 0, 0);
        }
      }
    }
  }
  float* P = p.P + ((long)s * p.Z + z) * p.Cout * p.Cin;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int id = w * per_w + j;
    if (j < per_w && id < nblk) {
      const int cob = id / nbc, cib = id - cob * nbc;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        P[(long)(co0 + cob * 16 + 4 * g + e) * p.Cin + ci0 + cib * 16 + r] = acc[j][e];
    }
  }
  if (bias_block && tid < tco) p.Pb[((long)s * p.nph + ph) * p.Cout + co0 + tid] = bsum;
}

// G = sum over the S partials, in order, in the parameter's layout: (Cout, Cin, taps), or (Cin, Cout, 2 up) for a transposed conv,
// whose kernel index j = d up + r + up / 2 (d in {-1, 0, 1}) is phase r, tap 1 - d.  dbias[co] = sum over the partials and the phases.
__global__ void voc_wgrad_reduce_kernel(const float* P, const float* Pb, float* G, float* dbias, int S, int Z, int nph, int Cout, int Cin,
                                        int taps, int up, long nG) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nG) {
    int co, ci, z;
    if (up == 1) {
      z = (int)(e % taps);
      ci = (int)((e / taps) % Cin);
      co = (int)(e / ((long)taps * Cin));
    } else {
      const int K = 2 * up, j = (int)(e % K), q = j - up / 2;
      co = (int)((e / K) % Cout);
      ci = (int)(e / ((long)K * Cout));
      const int d = q < 0 ? -1 : (q >= up ? 1 : 0), r = q - d * up;
      z = r * 3 + (1 - d);
    }
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += P[(((long)s * Z + z) * Cout + co) * Cin + ci];
    G[e] = a;
  } else if (dbias && e < nG + Cout) {
    const int co = (int)(e - nG);
    float a = 0.f;
    for (int s = 0; s < S; ++s)
      for (int ph = 0; ph < nph; ++ph) a += Pb[((long)s * nph + ph) * Cout + co];
    dbias[co] = a;
  }
}

// dX = acc( fma(scale lrelu'(Xs), U, R) ) on (B, N, C) channels-last tensors of one batch stride; rows at or past the length: 0
__global__ void __launch_bounds__(THREADS) voc_act_bwd_kernel(const float* Xs, const float* U, const float* R, float* dX, const int* frames,
                                                              int scale, int N, int C, float gscale, int acc, long total4) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= total4) return;
  const long row = e * 4 / C;
  const int b = (int)(row / N), n = (int)(row - (long)b * N);
  const int len = min(frames[b] * scale, N);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n < len) {
    const float4 u = reinterpret_cast<const float4*>(U)[e];
    float4 sl = make_float4(gscale, gscale, gscale, gscale);
    if (Xs) {
      const float4 x = reinterpret_cast<const float4*>(Xs)[e];
      sl.x *= dlrelu(x.x); sl.y *= dlrelu(x.y); sl.z *= dlrelu(x.z); sl.w *= dlrelu(x.w);
    }
    if (R) v = reinterpret_cast<const float4*>(R)[e];
    if (acc) {
      const float4 o = reinterpret_cast<const float4*>(dX)[e];
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    v.x = __builtin_fmaf(sl.x, u.x, v.x); v.y = __builtin_fmaf(sl.y, u.y, v.y);
    v.z = __builtin_fmaf(sl.z, u.z, v.z); v.w = __builtin_fmaf(sl.w, u.w, v.w);
  }
  reinterpret_cast<float4*>(dX)[e] = v;
}

// conv_post backward: one workgroup per PPASS x PT samples of one batch row.  Per pass: dz (with 3 samples of halo either side) and
// the PT rows of x in LDS; thread i writes dX of sample i; thread (c, t) adds the pass's PT terms of dw[c][t], thread 7 C those of db.
// P[workgroup][7 C + 1]: the partial sums.
template <int C>
__global__ void __launch_bounds__(THREADS) voc_post_bwd_kernel(const float* X, long sxb, const float* W, const float* Y, const float* dY,
                                                               int ldy, float* dX, float* P, const int* frames, int scale, int N) {
  __shared__ __attribute__((aligned(16))) float xs[PT * C];
  __shared__ float dz[PT + 6];
  __shared__ float ws[C * 7];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int len = min(frames[b] * scale, N);
  for (int e = tid; e < C * 7; e += THREADS) ws[e] = W[e];
  const float* x = X + (long)b * sxb;
  float* dx = dX + (long)b * sxb;
  const int c = tid / 7, t = tid - c * 7;
  double part = 0.0;      // dw and db are sums over every sample that cancel heavily (db: a single number): they are added in double
  for (int pass = 0; pass < PPASS; ++pass) {
    const int s0 = (blockIdx.x * PPASS + pass) * PT;
    if (s0 >= N) break;
    __syncthreads();
    for (int i = tid; i < PT + 6; i += THREADS) {
      const int n = s0 - 3 + i;
      float v = 0.f;
      if (n >= 0 && n < len) {
        const float y = Y[(long)b * ldy + n];
        v = dY[(long)b * ldy + n] * (1.f - y * y);
      }
      dz[i] = v;
    }
    for (int e = tid; e < PT * (C / 4); e += THREADS) {
      const int rr = e / (C / 4), n = s0 + rr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < len) v = reinterpret_cast<const float4*>(x + (long)n * C)[e - rr * (C / 4)];
      reinterpret_cast<float4*>(xs)[e] = v;
    }
    __syncthreads();
    const int n = s0 + tid;
    if (n < N) {
      float d[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) d[k] = dz[tid + 6 - k];            // dz[n + 3 - k]
      for (int c4 = 0; c4 < C / 4; ++c4) {
        const float4 xv = reinterpret_cast<const float4*>(xs)[tid * (C / 4) + c4];
        const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float a = 0.f;
#pragma unroll
          for (int k = 0; k < 7; ++k) a = __builtin_fmaf(d[k], ws[(4 * c4 + i) * 7 + k], a);
          o[i] = n < len ? dlrelu(xe[i]) * a : 0.f;
        }
        reinterpret_cast<float4*>(dx + (long)n * C)[c4] = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
    if (tid < C * 7) {                                         // dw[c][t] = sum_m lrelu(x[m][c]) dz[m + 3 - t]
      for (int m = 0; m < PT; ++m) part = __builtin_fma((double)lrelu(xs[m * C + c]), (double)dz[m + 6 - t], part);
    } else if (tid == C * 7) {
      for (int m = 0; m < PT; ++m) part += (double)dz[m + 3];
    }
  }
  if (tid <= C * 7) P[((long)b * gridDim.x + blockIdx.x) * (C * 7 + 1) + tid] = (float)part;
}

// dW[e] (e < 7 C) and db = the nP partial sums added in order
__global__ void voc_post_bwd_reduce_kernel(const float* P, float* dW, float* db, int nP, int M) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M) return;
  double a = 0.0;
  for (int s = 0; s < nP; ++s) a += (double)P[(long)s * M + e];
  if (e < M - 1) dW[e] = (float)a; else db[0] = (float)a;
}

bool voc_wgrad_shape_ok(int B, int N, int Cin, int Cout, int taps, int dil, int up) {
  if (!(B > 0 && N > 0 && Cin >= 16 && Cin % 16 == 0 && Cin <= 512 && Cout >= 16 && Cout % 16 == 0 && Cout <= 512)) return false;
  if (up == 1) return taps >= 1 && taps % 2 == 1 && taps <= 11 && dil >= 1 && dil * (taps - 1) <= 72;
  return taps == 3 && dil == 1 && up >= 2 && up % 2 == 0 && up <= 8;
}

}  // namespace

extern "C" {

int dx_voc_wgrad_size(int B, int N, int Cin, int Cout, int taps, int up, long* bytes) {
  DX_REQUIRE(bytes, "dx_voc_wgrad_size: null output");
  WgradPlan pl;
  DX_REQUIRE(voc_wgrad_shape_ok(B, N, Cin, Cout, taps, 1, up) && voc_wgrad_plan(B, N, Cin, Cout, taps, up, pl),
             "dx_voc_wgrad_size: bad shape (Cin, Cout multiples of 16 up to 512; odd taps <= 11, or taps 3 with an even up <= 8)");
  *bytes = (pl.g_elems + pl.b_elems) * 4;
  return DX_OK;
}

int dx_voc_wgrad(const float* X, long sxb, long sxn, long sxc, const float* dY, long dyb, int ldy, int dyc, float* G, float* dbias,
                 float* workspace, long workspace_bytes, const int* frames, int scale, int B, int N, int Cin, int Cout, int taps, int dil,
                 int up, int act, void* stream) {
  DX_REQUIRE(X && dY && G && workspace && frames, "dx_voc_wgrad: null pointer");
  DX_REQUIRE(voc_wgrad_shape_ok(B, N, Cin, Cout, taps, dil, up) && scale > 0,
             "dx_voc_wgrad: bad shape (Cin, Cout multiples of 16 up to 512; odd taps <= 11 with dilation (taps - 1) <= 72, or the "
             "three-tap view of a transposed conv: taps 3, dilation 1, even up <= 8)");
  DX_REQUIRE(act == 0 || act == 1, "dx_voc_wgrad: bad act (0 identity, 1 leaky-ReLU)");
  const int nph = up > 1 ? up : 1;
  DX_REQUIRE(dyc >= 0 && dyc % 4 == 0 && ldy % 4 == 0 && dyb % 4 == 0 && dx_aligned16(dY) && (long)dyc + (long)nph * Cout <= ldy &&
                 (long)N * ldy <= dyb,
             "dx_voc_wgrad: dY needs offset, row and batch strides %% 4 == 0, a 16-byte aligned pointer, rows that hold offset + up Cout "
             "channels and a batch stride that holds N rows");
  DX_REQUIRE(sxn > 0 && sxc > 0 && sxb >= 0, "dx_voc_wgrad: bad strides of X");
  DX_REQUIRE(sxc != 1 || sxn < Cin || (sxn % 4 == 0 && sxb % 4 == 0 && dx_aligned16(X)),
             "dx_voc_wgrad: channels-last X needs strides %% 4 == 0 and a 16-byte aligned pointer");
  WgradPlan pl;
  DX_REQUIRE(voc_wgrad_plan(B, N, Cin, Cout, taps, up, pl), "dx_voc_wgrad: too many tiles");
  DX_REQUIRE(workspace_bytes >= (pl.g_elems + pl.b_elems) * 4 && dx_aligned16(workspace), "dx_voc_wgrad: workspace smaller than dx_voc_wgrad_size reports");
  WgradArgs a;
  a.X = X; a.sxb = sxb; a.sxn = sxn; a.sxc = sxc;
  a.dY = dY; a.dyb = dyb; a.ldy = ldy; a.dyc = dyc;
  a.P = workspace; a.Pb = workspace + pl.g_elems;
  a.frames = frames; a.scale = scale;
  a.N = N; a.Cin = Cin; a.Cout = Cout; a.taps = taps; a.dil = dil; a.pad = dil * (taps - 1) / 2; a.up = up; a.act = act;
  a.tilesN = pl.tilesN; a.total = pl.total; a.per = pl.per; a.nci = pl.nci; a.Z = pl.Z; a.nph = pl.nph;
  hipStream_t s = (hipStream_t)stream;
  const size_t smem = (size_t)2 * WT * tile_ld(WC) * sizeof(float);
  hipLaunchKernelGGL(voc_wgrad_kernel, dim3(pl.S, pl.nco * pl.nci, pl.Z), dim3(THREADS), smem, s, a);
  DX_LAUNCH_CHECK("dx_voc_wgrad");
  const long nG = (long)Cout * Cin * (up > 1 ? 2 * up : taps);
  hipLaunchKernelGGL(voc_wgrad_reduce_kernel, dim3((unsigned)((nG + Cout + 255) / 256)), dim3(256), 0, s, a.P, a.Pb, G, dbias, pl.S, pl.Z,
                     pl.nph, Cout, Cin, taps, up, nG);
  DX_LAUNCH_CHECK("dx_voc_wgrad (reduce)");
  return DX_OK;
}

int dx_voc_act_bwd(const float* Xs, const float* U, const float* R, float* dX, const int* frames, int scale, int B, int N, int C,
                   float gscale, int acc, void* stream) {
  DX_REQUIRE(U && dX && frames, "dx_voc_act_bwd: null pointer");
  DX_REQUIRE(B > 0 && N > 0 && scale > 0 && C > 0 && C % 4 == 0, "dx_voc_act_bwd: bad shape (C %% 4 == 0)");
  DX_REQUIRE(acc == 0 || acc == 1, "dx_voc_act_bwd: bad acc (0 write, 1 add)");
  DX_REQUIRE(dx_aligned16(U) && dx_aligned16(dX) && dx_aligned16(Xs) && dx_aligned16(R), "dx_voc_act_bwd: pointers must be 16-byte aligned");
  const long total4 = (long)B * N * C / 4;
  hipLaunchKernelGGL(voc_act_bwd_kernel, dim3((unsigned)((total4 + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, Xs, U, R, dX,
                     frames, scale, N, C, gscale, acc, total4);
  DX_LAUNCH_CHECK("dx_voc_act_bwd");
  return DX_OK;
}

int dx_voc_post_bwd_size(int B, int N, int C, long* bytes) {
  DX_REQUIRE(bytes, "dx_voc_post_bwd_size: null output");
  DX_REQUIRE(B > 0 && N > 0 && (C == 16 || C == 32), "dx_voc_post_bwd_size: bad shape (C in {16, 32})");
  *bytes = (long)B * dx_cdiv(N, PT * PPASS) * (C * 7 + 1) * 4;
  return DX_OK;
}

int dx_voc_post_bwd(const float* X, long sxb, const float* W, const float* Y, const float* dY, int ldy, float* dX, float* dW, float* db,
                    float* workspace, long workspace_bytes, const int* frames, int scale, int B, int N, int C, void* stream) {
  DX_REQUIRE(X && W && Y && dY && dX && dW && db && workspace && frames, "dx_voc_post_bwd: null pointer");
  DX_REQUIRE(C == 16 || C == 32, "dx_voc_post_bwd: bad channel count (C in {16, 32})");
  DX_REQUIRE(B > 0 && N > 0 && scale > 0 && ldy >= N && sxb % 4 == 0 && sxb >= (long)N * C && dx_aligned16(X) && dx_aligned16(dX) && X != dX,
             "dx_voc_post_bwd: bad shape (ldy >= N, sxb %% 4 == 0 and holding N rows, 16-byte aligned X and dX, dX not X)");
  const int nbx = dx_cdiv(N, PT * PPASS), M = C * 7 + 1;
  DX_REQUIRE(workspace_bytes >= (long)B * nbx * M * 4, "dx_voc_post_bwd: workspace smaller than dx_voc_post_bwd_size reports");
  hipStream_t s = (hipStream_t)stream;
  if (C == 32)
    hipLaunchKernelGGL(voc_post_bwd_kernel<32>, dim3(nbx, B), dim3(THREADS), 0, s, X, sxb, W, Y, dY, ldy, dX, workspace, frames, scale, N);
  else
    hipLaunchKernelGGL(voc_post_bwd_kernel<16>, dim3(nbx, B), dim3(THREADS), 0, s, X, sxb, W, Y, dY, ldy, dX, workspace, frames, scale, N);
  DX_LAUNCH_CHECK("dx_voc_post_bwd");
  hipLaunchKernelGGL(voc_post_bwd_reduce_kernel, dim3(1), dim3(256), 0, s, workspace, dW, db, B * nbx, M);
  DX_LAUNCH_CHECK("dx_voc_post_bwd (reduce)");
  return DX_OK;
}

}  // extern "C"
