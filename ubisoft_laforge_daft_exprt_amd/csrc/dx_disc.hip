// HiFi-GAN discriminators (reference src/daft_exprt/vocoder/discriminators.py), forward only: the Multi-Period and Multi-Scale
// discriminators' layers and the three GAN losses.
//
// Activations are fp32, channels-last.  A "row" is one independent 1-D signal: a batch row of the MSD ([B][T][C]) or one column of
// the MPD's period-folded tensor ([B][H][p][C]: row = (b, column), position stride p * C).  Rows are addressed by explicit strides
// (batch stride, column stride, position stride), so the folded tensor is never transposed or copied.  Real and generated audio are
// rows of one batch: every layer is one launch over both.
//
// dx_disc_conv: a strided, grouped, k-tap Conv1d as an implicit GEMM over a tile of 64 output positions of ONE row and 64 * NI output
// channels:   out[m][n] = sum_t sum_c A[m * stride - pad + t][c] * W[n][c][t],   c over the input channels of n's group.
// The input window ((64 - 1) * stride + taps positions) is staged in LDS, up to 64 channels of a group at a time (a "chunk"); the GEMM's
// K axis inside a chunk is k = t * cg + c (cg = channels per chunk and group), zero-padded to the MFMA k step INSIDE THE PACK (the
// smallest layer, 8 channels per group x 41 taps, has K = 328).  A workgroup whose 64 output channels span several groups (16 or 32
// output channels per group) stages all their input channels side by side; each wave then reads its own group's columns.  The window
// is stored de-interleaved by stride phase (LDS row of window position q = (q % stride) * RP + q / stride), so the 16 lanes of an MFMA
// row block read 16 CONSECUTIVE LDS rows whatever the stride.  Exact-f32 mode: v_mfma_f32_16x16x4_f32; bf16 mode:
// v_mfma_f32_16x16x32_bf16; fp32 accumulation, bias and leaky-ReLU in the epilogue, one store per output element.
//
// No atomics anywhere: every output element and every loss is summed in an order fixed by the shapes alone.
#include "dx_disc_tile.h"

namespace {

constexpr int KC = 64;              // input channels of one group per LDS chunk, at most
constexpr int LOSS_CHUNK = 16384;   // elements per partial sum of dx_disc_losses

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * DISC_SLOPE; }

// chunk geometry shared by the pack and the kernel: cg channels of a group per chunk, nchunks chunks, KST k steps per chunk
struct PackGeom { int cg, lg, nchunks, KST; };
bool pack_geom(int Cin_g, int taps, int bf16, PackGeom* q) {
  if (Cin_g <= 0 || taps <= 0) return false;
  const int cg = Cin_g < KC ? Cin_g : KC;
  if (cg < 8 || (cg & (cg - 1)) != 0 || Cin_g % cg != 0) return false;
  q->cg = cg;
  q->lg = __builtin_ctz(cg);
  q->nchunks = Cin_g / cg;
  q->KST = dx_cdiv(taps * cg, bf16 ? 32 : 16);
  return true;
}

struct ConvArgs {
  const float* X; long sxb, sxr, sxn;
  const uint4* Wp; const float* bias;
  float* Y; long syb, syr, syn;
  int rdiv, N, Nout, Cin_g, Cout_g, taps, stride, inv_stride, pad, cg, lg, nchunks, KST, act;
};

// NI: 16-wide column blocks per wave (the workgroup covers 64 * NI output channels, all of one group when NI > 1)
template <bool BF, int NI>
__global__ void __launch_bounds__(THREADS) disc_conv_kernel(ConvArgs p) {
  typedef DxMmaOp<BF> Op;
  typedef typename Op::T T;
  extern __shared__ __attribute__((aligned(16))) unsigned char disc_smem[];
  T* A = reinterpret_cast<T*>(disc_smem);
  const int row = blockIdx.y, m0 = blockIdx.x * DT, co0 = blockIdx.z * (NI * 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const float* X = p.X + disc_row_offset(row, p.rdiv, p.sxb, p.sxr);
  float* Y = p.Y + disc_row_offset(row, p.rdiv, p.syb, p.syr);
  const int grp0 = co0 / p.Cout_g;
  const int ngrp = p.Cout_g >= NI * 64 ? 1 : (NI * 64) / p.Cout_g;
  const int cw = ngrp * p.cg, lda = cw + Op::PAD;
  const int rows = (DT - 1) * p.stride + p.taps, RP = (rows + p.stride - 1) / p.stride;
  const int coff = ((co0 + w * 16) / p.Cout_g - grp0) * p.cg;      // this wave's group inside the staged channels
  // LDS row of window position q (a tap, or a staged row): de-interleaved by stride phase, (q % stride) * RP + q / stride
  const auto lrow = [&](int q) {
    const int qd = (q * p.inv_stride) >> 16;
    return (q - qd * p.stride) * RP + qd;
  };
  f32x4 acc[NI][4] = {}, part[NI][4] = {};
  for (int ch = 0; ch < p.nchunks; ++ch) {
    __syncthreads();
    disc_stage<BF>(A, lda, X + (grp0 * p.Cin_g + ch * p.cg), p.sxn, m0 * p.stride - p.pad, p.N, rows, cw >> 2, lrow);
    __syncthreads();
    disc_chunk_mma<BF>(A, lda, coff, p.Wp + ((long)(co0 / 16 + w) * p.nchunks + ch) * p.KST * 64, 4L * p.nchunks * p.KST * 64, p.KST,
                       p.taps * p.cg, p.lg, p.cg - 1, lrow, acc, part);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = co0 + (w + 4 * i) * 16 + r;
    const float bn = p.bias[n];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + j * 16 + 4 * g + e;
        if (m >= p.Nout) continue;
        float v = (acc[i][j][e] + part[i][j][e]) + bn;
        if (p.act) v = lrelu(v);
        Y[(long)m * p.syn + n] = v;
      }
    }
  }
}

// Pack: [column block][chunk][k step][lane][VEC]; lane (n = l & 15, g = l >> 4) element v holds k = ks * KS + g * VEC + v of output
// channel nb * 16 + n, k = t * cg + c the tap and the channel inside the chunk; zero at k >= taps * cg.  W is (Cout, Cin_g, taps).
template <bool BF>
__global__ void disc_pack_kernel(const float* W, void* out, int Cin_g, int taps, PackGeom q, long total) {
  typedef DxMmaOp<BF> Op;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  DiscPackIdx x = disc_pack_lane<BF>(e);
  disc_pack_step<BF>(x, q.KST, q.nchunks);
  float val = 0.f;
  if (x.k < taps * q.cg) {
    const int t = x.k >> q.lg, c = x.ch * q.cg + (x.k & (q.cg - 1));
    val = W[((long)x.n * Cin_g + c) * taps + t];
  }
  reinterpret_cast<typename Op::T*>(out)[e] = Op::cvt(val);
}

long pack_elems(int Cout, const PackGeom& q, int bf16) { return (long)(Cout / 16) * q.nchunks * q.KST * 64 * (bf16 ? 8 : 4); }

template <bool BF, int NI>
int launch_conv(const ConvArgs& a, int rows, int Cout, hipStream_t s) {
  typedef DxMmaOp<BF> Op;
  const int ngrp = a.Cout_g >= NI * 64 ? 1 : (NI * 64) / a.Cout_g;
  const int win = (DT - 1) * a.stride + a.taps, RP = dx_cdiv(win, a.stride);
  const size_t smem = (size_t)RP * a.stride * (ngrp * a.cg + Op::PAD) * sizeof(typename Op::T);
  DX_REQUIRE(smem <= 64 * 1024, "dx_disc_conv: unsupported shape (the input window of a tile needs %zu bytes of LDS, more than 64 KB)", smem);
  hipLaunchKernelGGL((disc_conv_kernel<BF, NI>), dim3(dx_cdiv(a.Nout, DT), rows, Cout / (NI * 64)), dim3(THREADS), smem, s, a);
  DX_LAUNCH_CHECK("dx_disc_conv");
  return DX_OK;
}

template <bool BF>
int dispatch_conv(const ConvArgs& a, int rows, int Cout, hipStream_t s) {
  if (a.Cout_g % 256 == 0) return launch_conv<BF, 4>(a, rows, Cout, s);
  if (a.Cout_g % 128 == 0) return launch_conv<BF, 2>(a, rows, Cout, s);
  return launch_conv<BF, 1>(a, rows, Cout, s);
}

// The Cin = 1 first layers: Y[b][m][w][co] = lrelu(bias[co] + sum_t W[co][t] * x[b][(m stride - pad + t) p + w]); positions outside
// [0, H) are the conv's zero padding, samples at or past T the right reflect padding (index 2 (T - 1) - i).  One output per thread.
__global__ void __launch_bounds__(THREADS) disc_first_kernel(const float* x, long sxb, int T, const float* W, const float* bias, float* Y,
                                                             int p, int H, int Hout, int Cout, int taps, int stride, int pad, long total) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= total) return;
  const int co = (int)(e % Cout);
  long pos = e / Cout;
  const int wc = (int)(pos % p); pos /= p;
  const int m = (int)(pos % Hout);
  const long b = pos / Hout;
  const float* xr = x + b * sxb;
  const float* wr = W + (long)co * taps;
  float acc = 0.f;
  for (int t = 0; t < taps; ++t) {
    const int h = m * stride - pad + t;
    if (h < 0 || h >= H) continue;
    long i = (long)h * p + wc;
    if (i >= T) i = 2L * (T - 1) - i;
    acc = __builtin_fmaf(xr[i], wr[t], acc);
  }
  Y[e] = lrelu(acc + bias[co]);
}

// acc + comp += a * b with the rounding errors of the product and of the sum carried in comp (fp32 only: the product's error from one
// FMA, the sum's from Knuth's two-sum), so a long dot product keeps fp32's full precision whatever its length.
__device__ __forceinline__ void dot2_step(float a, float b, float& acc, float& comp) {
  const float p = a * b, pe = __builtin_fmaf(a, b, -p);
  const float s = acc + p, bb = s - acc;
  comp += ((acc - (s - bb)) + (p - bb)) + pe;
  acc = s;
}

// The Cout = 1 last layers: one wave per output position; lane l sums channels 4 l + 256 j in order (compensated: the 3 x 1024 terms
// would otherwise cost the scores about half a digit against the fp32 reference), then a fixed butterfly over the lanes.
__global__ void __launch_bounds__(THREADS) disc_post_kernel(const float* X, long sxb, long sxr, long sxn, const float* W, const float* bias,
                                                            float* Y, long syb, long syr, long syn, int rdiv, int N, int C, int taps, long total) {
  const long id = (long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
  if (id >= total) return;
  const int lane = threadIdx.x & 63;
  const int row = (int)(id / N), m = (int)(id - (long)row * N);
  const int pad = (taps - 1) / 2;
  const float* x = X + disc_row_offset(row, rdiv, sxb, sxr);
  float acc = 0.f, comp = 0.f;
  for (int t = 0; t < taps; ++t) {
    const int n = m - pad + t;
    if (n < 0 || n >= N) continue;
    const float* xr = x + (long)n * sxn;
    for (int c = lane * 4; c < C; c += 256) {
      const float4 v = *reinterpret_cast<const float4*>(xr + c);
      dot2_step(v.x, W[(long)(c + 0) * taps + t], acc, comp);
      dot2_step(v.y, W[(long)(c + 1) * taps + t], acc, comp);
      dot2_step(v.z, W[(long)(c + 2) * taps + t], acc, comp);
      dot2_step(v.w, W[(long)(c + 3) * taps + t], acc, comp);
    }
  }
  acc = dx_wave_sum(acc + comp);
  if (lane == 0) Y[disc_row_offset(row, rdiv, syb, syr) + (long)m * syn] = acc + bias[0];
}

// AvgPool1d(4, 2, padding = 2), count_include_pad: y[j] = (x[2j-2] + x[2j-1] + x[2j] + x[2j+1]) / 4, zeros outside [0, T).
__global__ void __launch_bounds__(THREADS) disc_pool_kernel(const float* x, float* y, int T, int Tout, long total) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= total) return;
  const long row = e / Tout;
  const int j = (int)(e - row * Tout);
  const float* xr = x + row * T;
  float s = 0.f;
#pragma unroll
  for (int d = -2; d < 2; ++d) {
    const int i = 2 * j + d;
    s += (i >= 0 && i < T) ? xr[i] : 0.f;
  }
  y[e] = s * 0.25f;
}

// ---- losses -------------------------------------------------------------------------------------------------------------------
// code = kind + 2 * set; kind 0: a score pair (sums of (1 - r)^2, g^2, (1 - g)^2), kind 1: a feature-map pair (sum of |r - g|)
struct LossEntry { const float* r; const float* g; long count; long code; };

__device__ __forceinline__ float block_sum4(float v, float* sh) {       // 4 waves, summed in wave order by every thread
  v = dx_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// partial[(entry * nchunk + chunk) * 4 + {0, 1, 2}] = the sums over elements [chunk * LOSS_CHUNK, ...) of the entry
__global__ void __launch_bounds__(THREADS) disc_loss_partial_kernel(const LossEntry* tab, float* partial, int nchunk) {
  __shared__ float sh[4];
  const LossEntry en = tab[blockIdx.y];
  const long c0 = (long)blockIdx.x * LOSS_CHUNK;
  if (c0 >= en.count) return;
  const long c1 = en.count < c0 + LOSS_CHUNK ? en.count : c0 + LOSS_CHUNK;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (en.code & 1) {
    for (long i = c0 + threadIdx.x; i < c1; i += THREADS) s0 += fabsf(en.r[i] - en.g[i]);
  } else {
    for (long i = c0 + threadIdx.x; i < c1; i += THREADS) {
      const float a = 1.f - en.r[i], gv = en.g[i], b = 1.f - gv;
      s0 = __builtin_fmaf(a, a, s0); s1 = __builtin_fmaf(gv, gv, s1); s2 = __builtin_fmaf(b, b, s2);
    }
  }
  s0 = block_sum4(s0, sh); s1 = block_sum4(s1, sh); s2 = block_sum4(s2, sh);
  if (threadIdx.x == 0) {
    float* o = partial + ((long)blockIdx.y * nchunk + blockIdx.x) * 4;
    o[0] = s0; o[1] = s1; o[2] = s2;
  }
}

// out[3 s + {0, 1, 2}] = set s's {discriminator, generator, feature} totals; out[3 n_sets + 3 e + {0, 1, 2}] = entry e's means
// (score pair: mean (1 - r)^2, mean g^2, mean (1 - g)^2; feature-map pair: mean |r - g|, 0, 0).  Totals add the entries in table order,
// as the reference's `loss += ...` loops do; the feature total is doubled at the end.
__global__ void __launch_bounds__(THREADS) disc_loss_final_kernel(const LossEntry* tab, const float* partial, int nchunk, int n, int n_sets,
                                                                  float* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* terms = out + 3 * n_sets;
  for (int e = w; e < n; e += THREADS / 64) {
    const long count = tab[e].count;
    const long chunks = (count + LOSS_CHUNK - 1) / LOSS_CHUNK;
    const int used = chunks < nchunk ? (int)chunks : nchunk;           // count <= max_count is the caller's contract; never read past
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int c = lane; c < used; c += 64) {
      const float* q = partial + ((long)e * nchunk + c) * 4;
      s0 += q[0]; s1 += q[1]; s2 += q[2];
    }
    s0 = dx_wave_sum(s0); s1 = dx_wave_sum(s1); s2 = dx_wave_sum(s2);
    if (lane == 0) {
      const float cnt = (float)count;
      terms[3 * e + 0] = s0 / cnt; terms[3 * e + 1] = s1 / cnt; terms[3 * e + 2] = s2 / cnt;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n_sets) {
    const int s = threadIdx.x;
    float d = 0.f, gen = 0.f, fm = 0.f;
    for (int e = 0; e < n; ++e) {
      const long code = tab[e].code;
      if ((int)(code >> 1) != s) continue;
      if (code & 1) {
        fm += terms[3 * e];
      } else {
        d += terms[3 * e] + terms[3 * e + 1];
        gen += terms[3 * e + 2];
      }
    }
    out[3 * s + 0] = d; out[3 * s + 1] = gen; out[3 * s + 2] = fm * 2.f;
  }
}

}  // namespace

extern "C" {

int dx_disc_pack_size(int Cout, int Cin_g, int taps, int bf16, long* bytes) {
  DX_REQUIRE(bytes, "dx_disc_pack_size: null output");
  PackGeom q;
  DX_REQUIRE(Cout > 0 && Cout % 16 == 0 && (bf16 == 0 || bf16 == 1) && taps > 0 && taps <= 41 && pack_geom(Cin_g, taps, bf16, &q),
             "dx_disc_pack_size: bad shape (Cout %% 16 == 0; channels per group 8, 16, 32 or a multiple of 64; taps <= 41)");
  *bytes = pack_elems(Cout, q, bf16) * (bf16 ? 2 : 4);
  return DX_OK;
}

int dx_disc_pack(const float* W, void* Wp, int Cout, int Cin_g, int taps, int bf16, void* stream) {
  DX_REQUIRE(W && Wp, "dx_disc_pack: null pointer");
  PackGeom q;
  DX_REQUIRE(Cout > 0 && Cout % 16 == 0 && (bf16 == 0 || bf16 == 1) && taps > 0 && taps <= 41 && pack_geom(Cin_g, taps, bf16, &q),
             "dx_disc_pack: bad shape (Cout %% 16 == 0; channels per group 8, 16, 32 or a multiple of 64; taps <= 41)");
  const long total = pack_elems(Cout, q, bf16);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (bf16)
    hipLaunchKernelGGL(disc_pack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cin_g, taps, q, total);
  else
    hipLaunchKernelGGL(disc_pack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cin_g, taps, q, total);
  DX_LAUNCH_CHECK("dx_disc_pack");
  return DX_OK;
}

int dx_disc_conv(const float* X, long sxb, long sxr, long sxn, const void* Wp, const float* bias, float* Y, long syb, long syr, long syn,
                 int rows, int rdiv, int N, int Cin, int Cout, int groups, int taps, int stride, int pad, int act, int bf16,
                 void* stream) {
  DX_REQUIRE(X && Wp && bias && Y, "dx_disc_conv: null pointer");
  DX_REQUIRE((const void*)X != (const void*)Y, "dx_disc_conv: Y must not alias X (tiles read their neighbours' positions)");
  DX_REQUIRE(rows > 0 && rows <= 65535 && rdiv > 0 && N > 0 && Cin > 0 && Cout > 0 && groups > 0, "dx_disc_conv: non-positive size (rows <= 65535)");
  DX_REQUIRE(Cin % groups == 0 && Cout % groups == 0, "dx_disc_conv: Cin and Cout must be divisible by groups");
  DX_REQUIRE((bf16 == 0 || bf16 == 1) && (act == 0 || act == 1), "dx_disc_conv: bad act / bf16");
  DX_REQUIRE(taps > 0 && taps <= 41 && stride >= 1 && stride <= 4 && pad >= 0 && pad <= 20 && N + 2 * pad >= taps,
             "dx_disc_conv: unsupported taps / stride / pad (taps <= 41, stride <= 4, pad <= 20, N + 2 pad >= taps)");
  const int Cin_g = Cin / groups, Cout_g = Cout / groups;
  PackGeom q;
  DX_REQUIRE(pack_geom(Cin_g, taps, bf16, &q), "dx_disc_conv: unsupported shape (input channels per group 8, 16, 32 or a multiple of 64)");
  DX_REQUIRE(Cout % 64 == 0 && (Cout_g % 64 == 0 || ((Cout_g == 16 || Cout_g == 32) && q.nchunks == 1)) && Cout / 64 <= 65535,
             "dx_disc_conv: unsupported shape (Cout %% 64 == 0; output channels per group 16, 32 or a multiple of 64)");
  DX_REQUIRE(sxn % 4 == 0 && sxr % 4 == 0 && sxb % 4 == 0 && dx_aligned16(X),
             "dx_disc_conv: the input needs strides %% 4 == 0 and a 16-byte aligned X");
  ConvArgs a;
  a.X = X; a.sxb = sxb; a.sxr = sxr; a.sxn = sxn;
  a.Wp = reinterpret_cast<const uint4*>(Wp); a.bias = bias;
  a.Y = Y; a.syb = syb; a.syr = syr; a.syn = syn;
  a.rdiv = rdiv; a.N = N; a.Nout = (N + 2 * pad - taps) / stride + 1;
  a.Cin_g = Cin_g; a.Cout_g = Cout_g; a.taps = taps; a.stride = stride; a.inv_stride = 65536 / stride + 1; a.pad = pad;
  a.cg = q.cg; a.lg = q.lg; a.nchunks = q.nchunks; a.KST = q.KST; a.act = act;
  return bf16 ? dispatch_conv<true>(a, rows, Cout, (hipStream_t)stream) : dispatch_conv<false>(a, rows, Cout, (hipStream_t)stream);
}

int dx_disc_first(const float* x, long sxb, int T, const float* W, const float* bias, float* Y, int B, int p, int Cout, int taps,
                  int stride, int pad, void* stream) {
  DX_REQUIRE(x && W && bias && Y, "dx_disc_first: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && p > 0 && Cout > 0 && taps > 0 && stride > 0 && pad >= 0 && sxb >= T, "dx_disc_first: non-positive size (sxb >= T)");
  DX_REQUIRE(T % p == 0 || p - T % p < T, "dx_disc_first: the reflect padding (p - T %% p samples) must be shorter than the signal");
  const int H = dx_cdiv(T, p);
  DX_REQUIRE(H + 2 * pad >= taps, "dx_disc_first: unsupported shape (H + 2 pad >= taps)");
  const int Hout = (H + 2 * pad - taps) / stride + 1;
  const long total = (long)B * Hout * p * Cout;
  DX_REQUIRE((total + THREADS - 1) / THREADS <= 0x7fffffffL, "dx_disc_first: too many outputs for one launch");
  hipLaunchKernelGGL(disc_first_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                     x, sxb, T, W, bias, Y, p, H, Hout, Cout, taps, stride, pad, total);
  DX_LAUNCH_CHECK("dx_disc_first");
  return DX_OK;
}

int dx_disc_post(const float* X, long sxb, long sxr, long sxn, const float* W, const float* bias, float* Y, long syb, long syr, long syn,
                 int rows, int rdiv, int N, int C, int taps, void* stream) {
  DX_REQUIRE(X && W && bias && Y, "dx_disc_post: null pointer");
  DX_REQUIRE(rows > 0 && rdiv > 0 && N > 0 && C > 0 && C % 4 == 0 && taps > 0 && taps % 2 == 1,
             "dx_disc_post: bad shape (positive sizes, C %% 4 == 0, odd taps)");
  DX_REQUIRE(sxn % 4 == 0 && sxr % 4 == 0 && sxb % 4 == 0 && dx_aligned16(X), "dx_disc_post: the input needs strides %% 4 == 0 and a 16-byte aligned X");
  const long total = (long)rows * N;
  hipLaunchKernelGGL(disc_post_kernel, dim3((unsigned)((total + 3) / 4)), dim3(THREADS), 0, (hipStream_t)stream,
                     X, sxb, sxr, sxn, W, bias, Y, syb, syr, syn, rdiv, N, C, taps, total);
  DX_LAUNCH_CHECK("dx_disc_post");
  return DX_OK;
}

int dx_disc_pool(const float* x, float* y, int R, int T, void* stream) {
  DX_REQUIRE(x && y, "dx_disc_pool: null pointer");
  DX_REQUIRE(x != y, "dx_disc_pool: y must not alias x");
  DX_REQUIRE(R > 0 && T > 0, "dx_disc_pool: non-positive size");
  const int Tout = T / 2 + 1;
  const long total = (long)R * Tout;
  hipLaunchKernelGGL(disc_pool_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, x, y, T, Tout, total);
  DX_LAUNCH_CHECK("dx_disc_pool");
  return DX_OK;
}

int dx_disc_losses_workspace(long max_count, int n, long* floats) {
  DX_REQUIRE(floats, "dx_disc_losses_workspace: null output");
  DX_REQUIRE(max_count > 0 && n > 0, "dx_disc_losses_workspace: non-positive size");
  *floats = (long)n * ((max_count + LOSS_CHUNK - 1) / LOSS_CHUNK) * 4;
  return DX_OK;
}

int dx_disc_losses(const void* table, int n, int n_sets, long max_count, long total_count, float* partial, float* out, void* stream) {
  DX_REQUIRE(table && partial && out, "dx_disc_losses: null pointer");
  DX_REQUIRE(n > 0 && n <= 65535 && n_sets > 0 && n_sets <= THREADS && max_count > 0, "dx_disc_losses: non-positive size (n <= 65535, n_sets <= 256)");
  DX_REQUIRE(total_count >= max_count && total_count <= (long)n * max_count, "dx_disc_losses: total_count must lie in [max_count, n max_count]");
  const long nchunk = (max_count + LOSS_CHUNK - 1) / LOSS_CHUNK;
  DX_REQUIRE(nchunk <= 0x7fffffffL, "dx_disc_losses: max_count too large");
  const LossEntry* tab = reinterpret_cast<const LossEntry*>(table);
  hipLaunchKernelGGL(disc_loss_partial_kernel, dim3((unsigned)nchunk, n), dim3(THREADS), 0, (hipStream_t)stream, tab, partial, (int)nchunk);
  DX_LAUNCH_CHECK("dx_disc_losses");
  hipLaunchKernelGGL(disc_loss_final_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, tab, partial, (int)nchunk, n, n_sets, out);
  DX_LAUNCH_CHECK("dx_disc_losses");
  return DX_OK;
}

}  // extern "C"
