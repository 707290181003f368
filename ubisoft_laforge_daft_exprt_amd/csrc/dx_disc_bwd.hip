// HiFi-GAN discriminators, backward to the generated waveform: the gradient of the four generator-side losses
// (loss_gen_f, loss_fm_f, loss_gen_s, loss_fm_s) through the layers of dx_disc.hip.  Only the generated half of the batch has a
// gradient; the folded weights are constants.  Buffers are the forward's: fp32, channels-last, rows addressed by three strides.
//
// dx_disc_conv_dgrad: the data gradient of a strided, grouped, k-tap Conv1d.  The input positions are split by stride phase
// phi = (n + pad) mod s: with n + pad = s q + phi and t = phi + s u,
//     dX[n][ci] = sum_u sum_co dZ[q - u][co] * W[co][ci][phi + s u],      u < U = ceil((taps - phi) / s),  co over ci's group,
// a stride-1 convolution over dZ, so the LDS window of dZ is contiguous (63 + U positions for a tile of 64 q of ONE phase) and no
// MFMA multiplies a zero-stuffed position.  The GEMM's K axis is k = u * cgk + co (cgk = reduction channels per chunk), so a lane's 4
// (f32) or 8 (bf16) consecutive k are consecutive channels of one dZ position: one 16-byte LDS read.  The transposed weights come from
// a pack of their own, per phase.  The epilogue adds the feature-matching seed of the layer below and multiplies by its leaky-ReLU
// slope (read from the stored maps), so what is written is that layer's pre-activation gradient, once.
//
// No atomics, no scratch: every sum runs in an order fixed by the shapes alone.
#include "dx_disc_tile.h"

namespace {

constexpr int SUB = 8;              // lanes per waveform sample in dx_disc_first_bwd

__host__ __device__ __forceinline__ int taps_of_phase(int taps, int stride, int phase) { return (taps - phase + stride - 1) / stride; }
__host__ __device__ __forceinline__ int ksteps(int U, int cgk, int KS) { return (U * cgk + KS - 1) / KS; }

// cgk reduction channels (co) per chunk and 16-wide column block, nchunks chunks; ng groups per 64-column tile.  A column block of
// 8-channel groups spans two of them (span 2): its chunk holds both groups' co, block-diagonal in the pack.
struct DgGeom { int cgk, lg, nchunks, ng; };
bool dgrad_geom(int Cin, int Cout, int groups, DgGeom* q) {
  if (Cin <= 0 || Cout <= 0 || groups <= 0 || Cin % groups != 0 || Cout % groups != 0 || Cin % 16 != 0) return false;
  const int Cin_g = Cin / groups, Cout_g = Cout / groups;
  if (Cin_g != 8 && Cin_g % 16 != 0) return false;
  const long red = (long)Cout_g * (Cin_g == 8 ? 2 : 1);
  const int cgk = red < 64 ? (int)red : 64;
  if (cgk < 16 || (cgk & (cgk - 1)) != 0 || red % cgk != 0 || Cout_g % 4 != 0) return false;
  q->cgk = cgk;
  q->lg = __builtin_ctz(cgk);
  q->nchunks = (int)(red / cgk);
  if (Cin_g % 64 == 0 || (groups == 1 && Cin < 64)) {
    q->ng = 1;
  } else {
    if (64 % Cin_g != 0 || Cin % 64 != 0 || q->nchunks != 1) return false;
    q->ng = 64 / Cin_g;
  }
  return true;
}

long dgrad_pack_elems(int Cin, int taps, int stride, const DgGeom& q, int bf16) {
  long steps = 0;
  for (int f = 0; f < stride; ++f) steps += ksteps(taps_of_phase(taps, stride, f), q.cgk, bf16 ? 32 : 16);
  return steps * (Cin / 16) * q.nchunks * 64 * (bf16 ? 8 : 4);
}

struct DgArgs {
  const float* dZ; long szb, szr, szn;
  const uint4* Wp;
  float* dX; const float* R; const float* G; long sxb, sxr, sxn;
  const float* gw; float fm_scale;
  int rdiv, N, Nout, Cin, Cin_g, Cout_g, taps, stride, pad, cgk, lg, nchunks, ng, epi, qlo;
};

__device__ __forceinline__ float seeded(float v, float seed, float rv, float gv) {
  const float d = gv - rv;
  const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return __builtin_fmaf(seed, sg, v) * (gv > 0.f ? 1.f : DISC_SLOPE);
}

// NI: 16-wide column blocks per wave (the workgroup covers 64 * NI input channels, all of one group when NI > 1)
template <bool BF, int NI>
__global__ void __launch_bounds__(THREADS) disc_dgrad_kernel(DgArgs p) {
  typedef DxMmaOp<BF> Op;
  typedef typename Op::T T;
  extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
  T* A = reinterpret_cast<T*>(dg_smem);
  const int row = blockIdx.y, phase = blockIdx.z % p.stride, ci0 = (blockIdx.z / p.stride) * (NI * 64);
  const int q0 = p.qlo + blockIdx.x * DT;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const float* Z = p.dZ + disc_row_offset(row, p.rdiv, p.szb, p.szr);
  const long xoff = disc_row_offset(row, p.rdiv, p.sxb, p.sxr);
  const int U = taps_of_phase(p.taps, p.stride, phase), KST = ksteps(U, p.cgk, Op::KS);
  long poff = 0;                                                         // this phase's part of the pack, in lanes' 16-byte fragments
  for (int f = 0; f < phase; ++f) poff += ksteps(taps_of_phase(p.taps, p.stride, f), p.cgk, Op::KS);
  poff *= (long)(p.Cin / 16) * p.nchunks * 64;
  const int grp0 = ci0 / p.Cin_g;
  const int cw = p.ng == 1 ? p.cgk : p.ng * p.Cout_g, lda = cw + Op::PAD;
  const int coff = p.ng == 1 ? 0 : ((ci0 + w * 16) / p.Cin_g - grp0) * p.Cout_g;   // this wave's groups inside the staged channels
  const bool active = ci0 + w * 16 < p.Cin;                              // a 16- or 32-channel dense layer leaves waves without columns
  const int top = U - 1;             // window row of dZ position q - u: top - u (spelled U - 1 - u it costs the k loop an instruction)
  f32x4 acc[NI][4] = {}, part[NI][4] = {};
  for (int ch = 0; ch < p.nchunks; ++ch) {
    __syncthreads();
    disc_stage<BF>(A, lda, Z + (grp0 * p.Cout_g + ch * p.cgk), p.szn, q0 - (U - 1), p.Nout, DT - 1 + U, cw >> 2, [](int rr) { return rr; });
    __syncthreads();
    if (!active) continue;
    disc_chunk_mma<BF>(A, lda, coff, p.Wp + poff + ((long)(ci0 / 16 + w) * p.nchunks + ch) * KST * 64, 4L * p.nchunks * KST * 64, KST,
                       U * p.cgk, p.lg, p.cgk - 1, [=](int u) { return top - u; }, acc, part);
  }
  if (!active) return;
  const float seed = p.epi ? p.gw[0] * p.fm_scale : 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int ci = ci0 + (w + 4 * i) * 16 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = (q0 + j * 16 + 4 * g + e) * p.stride + phase - p.pad;
        if (n < 0 || n >= p.N) continue;
        const long off = xoff + (long)n * p.sxn + ci;
        float v = acc[i][j][e] + part[i][j][e];
        if (p.epi) v = seeded(v, seed, p.R[off], p.G[off]);
        p.dX[off] = v;
      }
    }
  }
}

// Pack: [phase][column block][chunk][k step][lane][VEC]; lane (n = l & 15, g = l >> 4) element v holds k = ks * KS + g * VEC + v of
// input channel ci = nb * 16 + n: k = u * cgk + c is tap phase + stride u and output channel (first group of the block) * Cout_g +
// chunk * cgk + c; zero past the phase's taps and where that output channel is not in ci's group.  W is (Cout, Cin_g, taps).
template <bool BF>
__global__ void disc_dgrad_pack_kernel(const float* W, void* out, int Cin, int Cin_g, int Cout_g, int taps, int stride, DgGeom q, long total) {
  typedef DxMmaOp<BF> Op;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  DiscPackIdx x = disc_pack_lane<BF>(e);
  int phase = 0, U = 0, KST = 0;
  for (; phase < stride; ++phase) {
    U = taps_of_phase(taps, stride, phase);
    KST = ksteps(U, q.cgk, Op::KS);
    const long per = (long)(Cin / 16) * q.nchunks * KST;
    if (x.f < per) break;
    x.f -= per;
  }
  disc_pack_step<BF>(x, KST, q.nchunks);
  const int ci = x.n, u = x.k >> q.lg, c = x.k & (q.cgk - 1), t = phase + stride * u;
  const int co = ((x.nb * 16) / Cin_g) * Cout_g + x.ch * q.cgk + c;
  float val = 0.f;
  if (u < U && t < taps && co / Cout_g == ci / Cin_g) val = W[((long)co * Cin_g + ci % Cin_g) * taps + t];
  reinterpret_cast<typename Op::T*>(out)[e] = Op::cvt(val);
}

template <bool BF, int NI>
int launch_dgrad(const DgArgs& a, int rows, hipStream_t s) {
  typedef DxMmaOp<BF> Op;
  const int cw = a.ng == 1 ? a.cgk : a.ng * a.Cout_g;
  const int U0 = taps_of_phase(a.taps, a.stride, 0);
  const size_t smem = (size_t)(DT - 1 + U0) * (cw + Op::PAD) * sizeof(typename Op::T);
  DX_REQUIRE(smem <= 64 * 1024, "dx_disc_conv_dgrad: unsupported shape (the dZ window of a tile needs %zu bytes of LDS, more than 64 KB)", smem);
  const int nq = (a.N - 1 + a.pad) / a.stride - a.qlo + 1;
  const long gz = (long)dx_cdiv(a.Cin, NI * 64) * a.stride;
  DX_REQUIRE(gz <= 65535, "dx_disc_conv_dgrad: too many channel tiles");
  hipLaunchKernelGGL((disc_dgrad_kernel<BF, NI>), dim3(dx_cdiv(nq, DT), rows, (unsigned)gz), dim3(THREADS), smem, s, a);
  DX_LAUNCH_CHECK("dx_disc_conv_dgrad");
  return DX_OK;
}

template <bool BF>
int dispatch_dgrad(const DgArgs& a, int rows, hipStream_t s) {
  if (a.Cin_g % 256 == 0) return launch_dgrad<BF, 4>(a, rows, s);
  if (a.Cin_g % 128 == 0) return launch_dgrad<BF, 2>(a, rows, s);
  return launch_dgrad<BF, 1>(a, rows, s);
}

__device__ __forceinline__ float score_seed(float sr, float sg, float wgen, float wfm) {
  const float d = sg - sr;
  const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return __builtin_fmaf(wgen, sg - 1.f, wfm * sgn);
}

// The Cout = 1 last layers, transposed: one thread per position and 4 channels; the score seed is recomputed per tap.
__global__ void __launch_bounds__(THREADS) disc_post_bwd_kernel(const float* Sr, const float* Sg, long ssb, long ssr, long ssn, const float* W,
                                                                float* dZ, const float* R, const float* G, long sxb, long sxr, long sxn,
                                                                const float* gw_gen, const float* gw_fm, float s_scale, float fm_scale,
                                                                int rdiv, int N, int C, int taps, int epi, long total) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= total) return;
  const int c4 = C >> 2;
  const int c = (int)(e % c4) * 4;
  long pos = e / c4;
  const int n = (int)(pos % N);
  const int row = (int)(pos / N);
  const int pad = (taps - 1) / 2;
  const long so = disc_row_offset(row, rdiv, ssb, ssr);
  const float wgen = gw_gen[0] * s_scale, wfm = gw_fm[0] * s_scale;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int t = 0; t < taps; ++t) {
    const int m = n + pad - t;
    if (m < 0 || m >= N) continue;
    const float ds = score_seed(Sr[so + (long)m * ssn], Sg[so + (long)m * ssn], wgen, wfm);
    a0 = __builtin_fmaf(ds, W[(long)(c + 0) * taps + t], a0);
    a1 = __builtin_fmaf(ds, W[(long)(c + 1) * taps + t], a1);
    a2 = __builtin_fmaf(ds, W[(long)(c + 2) * taps + t], a2);
    a3 = __builtin_fmaf(ds, W[(long)(c + 3) * taps + t], a3);
  }
  const long off = disc_row_offset(row, rdiv, sxb, sxr) + (long)n * sxn + c;
  if (epi) {
    const float seed = gw_fm[0] * fm_scale;
    const float4 rv = *reinterpret_cast<const float4*>(R + off), gv = *reinterpret_cast<const float4*>(G + off);
    a0 = seeded(a0, seed, rv.x, gv.x); a1 = seeded(a1, seed, rv.y, gv.y);
    a2 = seeded(a2, seed, rv.z, gv.z); a3 = seeded(a3, seed, rv.w, gv.w);
  }
  *reinterpret_cast<float4*>(dZ + off) = make_float4(a0, a1, a2, a3);
}

// The Cin = 1 first layers, transposed: SUB lanes per waveform sample; lane l sums channels 4 l + 32 j of every contributing tap of
// the sample's own folded position, then of its mirrored position in the reflect-padded tail, in order; a fixed butterfly joins the
// lanes.  dZ [B][Hout][p][Cout], W (Cout, 1, taps).
__global__ void __launch_bounds__(THREADS) disc_first_bwd_kernel(const float* dZ, const float* W, float* dy, long sdb, int T, int p, int H,
                                                                 int Hout, int Cout, int taps, int stride, int pad, int accumulate, long total) {
  const long id = ((long)blockIdx.x * THREADS + threadIdx.x) / SUB;
  const int sub = threadIdx.x & (SUB - 1);
  const bool live = id < total;
  const long b = live ? id / T : 0;
  const int i = live ? (int)(id - b * T) : 0;
  float acc = 0.f;
  for (int which = 0; which < 2 && live; ++which) {
    const long P = which == 0 ? i : 2L * (T - 1) - i;
    if (which == 1 && (P < T || P >= (long)H * p)) continue;
    const int h = (int)(P / p), wc = (int)(P - (long)h * p);
    for (int t = 0; t < taps; ++t) {
      const int hm = h + pad - t;
      if (hm < 0) break;
      const int m = hm / stride;
      if (m * stride != hm || m >= Hout) continue;
      const float* zr = dZ + (((long)b * Hout + m) * p + wc) * Cout;
      for (int c = sub * 4; c < Cout; c += SUB * 4) {
        const float4 z = *reinterpret_cast<const float4*>(zr + c);
        acc = __builtin_fmaf(z.x, W[(long)(c + 0) * taps + t], acc);
        acc = __builtin_fmaf(z.y, W[(long)(c + 1) * taps + t], acc);
        acc = __builtin_fmaf(z.z, W[(long)(c + 2) * taps + t], acc);
        acc = __builtin_fmaf(z.w, W[(long)(c + 3) * taps + t], acc);
      }
    }
  }
#pragma unroll
  for (int off = 1; off < SUB; off <<= 1) acc += __shfl_xor(acc, off, 64);
  if (live && sub == 0) {
    float* o = dy + b * sdb + i;
    *o = accumulate ? *o + acc : acc;
  }
}

// AvgPool1d(4, 2, padding = 2) transposed: dx[i] = 0.25 (dy[i / 2] + dy[i / 2 + 1]), terms at or past Tout dropped.
__global__ void __launch_bounds__(THREADS) disc_pool_bwd_kernel(const float* dy, float* dx, int T, int Tout, int accumulate, long total) {
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= total) return;
  const long row = e / T;
  const int i = (int)(e - row * T), j = i >> 1;
  const float* yr = dy + row * Tout;
  float s = j < Tout ? yr[j] : 0.f;
  s += j + 1 < Tout ? yr[j + 1] : 0.f;
  s *= 0.25f;
  dx[e] = accumulate ? dx[e] + s : s;
}

bool dgrad_shape_ok(int Cin, int Cout, int groups, int taps, int stride, int bf16, DgGeom* q) {
  return (bf16 == 0 || bf16 == 1) && taps > 0 && taps <= 41 && stride >= 1 && stride <= 4 && taps >= stride && dgrad_geom(Cin, Cout, groups, q);
}

}  // namespace

extern "C" {

int dx_disc_dgrad_pack_size(int Cin, int Cout, int groups, int taps, int stride, int bf16, long* bytes) {
  DX_REQUIRE(bytes, "dx_disc_dgrad_pack_size: null output");
  DgGeom q;
  DX_REQUIRE(dgrad_shape_ok(Cin, Cout, groups, taps, stride, bf16, &q),
             "dx_disc_dgrad_pack_size: bad shape (Cin %% 16 == 0; input channels per group 8, 16, 32 or a multiple of 64; output channels per "
             "group 16, 32 or a multiple of 64; stride <= taps <= 41, stride <= 4)");
  *bytes = dgrad_pack_elems(Cin, taps, stride, q, bf16) * (bf16 ? 2 : 4);
  return DX_OK;
}

int dx_disc_dgrad_pack(const float* W, void* Wp, int Cin, int Cout, int groups, int taps, int stride, int bf16, void* stream) {
  DX_REQUIRE(W && Wp, "dx_disc_dgrad_pack: null pointer");
  DgGeom q;
  DX_REQUIRE(dgrad_shape_ok(Cin, Cout, groups, taps, stride, bf16, &q),
             "dx_disc_dgrad_pack: bad shape (Cin %% 16 == 0; input channels per group 8, 16, 32 or a multiple of 64; output channels per "
             "group 16, 32 or a multiple of 64; stride <= taps <= 41, stride <= 4)");
  const long total = dgrad_pack_elems(Cin, taps, stride, q, bf16);
  const dim3 grid((unsigned)((total + 255) / 256));
  if (bf16)
    hipLaunchKernelGGL(disc_dgrad_pack_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cin, Cin / groups, Cout / groups, taps, stride, q, total);
  else
    hipLaunchKernelGGL(disc_dgrad_pack_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, W, Wp, Cin, Cin / groups, Cout / groups, taps, stride, q, total);
  DX_LAUNCH_CHECK("dx_disc_dgrad_pack");
  return DX_OK;
}

int dx_disc_conv_dgrad(const float* dZ, long szb, long szr, long szn, const void* Wp, float* dX, const float* R, const float* G, long sxb,
                       long sxr, long sxn, const float* gw_fm, float fm_scale, int rows, int rdiv, int N, int Cin, int Cout, int groups,
                       int taps, int stride, int pad, int epilogue, int bf16, void* stream) {
  DX_REQUIRE(dZ && Wp && dX, "dx_disc_conv_dgrad: null pointer");
  DX_REQUIRE(epilogue == 0 || epilogue == 1, "dx_disc_conv_dgrad: bad epilogue flag");
  DX_REQUIRE(!epilogue || (R && G && gw_fm), "dx_disc_conv_dgrad: null pointer (the epilogue needs R, G and gw_fm)");
  DX_REQUIRE((const void*)dZ != (const void*)dX, "dx_disc_conv_dgrad: dX must not alias dZ (tiles read their neighbours' positions)");
  DX_REQUIRE(rows > 0 && rows <= 65535 && rdiv > 0 && N > 0 && Cin > 0 && Cout > 0 && groups > 0, "dx_disc_conv_dgrad: non-positive size (rows <= 65535)");
  DX_REQUIRE(Cin % groups == 0 && Cout % groups == 0, "dx_disc_conv_dgrad: Cin and Cout must be divisible by groups");
  DX_REQUIRE(bf16 == 0 || bf16 == 1, "dx_disc_conv_dgrad: bad bf16 flag");
  DX_REQUIRE(taps > 0 && taps <= 41 && stride >= 1 && stride <= 4 && taps >= stride && pad >= 0 && pad <= 20 && N + 2 * pad >= taps,
             "dx_disc_conv_dgrad: unsupported taps / stride / pad (stride <= taps <= 41, stride <= 4, pad <= 20, N + 2 pad >= taps)");
  DgGeom q;
  DX_REQUIRE(dgrad_geom(Cin, Cout, groups, &q),
             "dx_disc_conv_dgrad: unsupported shape (Cin %% 16 == 0; input channels per group 8, 16, 32 or a multiple of 64; output channels "
             "per group 16, 32 or a multiple of 64)");
  DX_REQUIRE(szn % 4 == 0 && szr % 4 == 0 && szb % 4 == 0 && dx_aligned16(dZ),
             "dx_disc_conv_dgrad: dZ needs strides %% 4 == 0 and a 16-byte aligned pointer");
  DgArgs a;
  a.dZ = dZ; a.szb = szb; a.szr = szr; a.szn = szn;
  a.Wp = reinterpret_cast<const uint4*>(Wp);
  a.dX = dX; a.R = R; a.G = G; a.sxb = sxb; a.sxr = sxr; a.sxn = sxn;
  a.gw = gw_fm; a.fm_scale = fm_scale;
  a.rdiv = rdiv; a.N = N; a.Nout = (N + 2 * pad - taps) / stride + 1;
  a.Cin = Cin; a.Cin_g = Cin / groups; a.Cout_g = Cout / groups; a.taps = taps; a.stride = stride; a.pad = pad;
  a.cgk = q.cgk; a.lg = q.lg; a.nchunks = q.nchunks; a.ng = q.ng; a.epi = epilogue; a.qlo = pad / stride;
  return bf16 ? dispatch_dgrad<true>(a, rows, (hipStream_t)stream) : dispatch_dgrad<false>(a, rows, (hipStream_t)stream);
}

int dx_disc_post_bwd(const float* Sr, const float* Sg, long ssb, long ssr, long ssn, const float* W, float* dZ, const float* R, const float* G,
                     long sxb, long sxr, long sxn, const float* gw_gen, const float* gw_fm, float s_scale, float fm_scale, int rows, int rdiv,
                     int N, int C, int taps, int epilogue, void* stream) {
  DX_REQUIRE(Sr && Sg && W && dZ && gw_gen && gw_fm, "dx_disc_post_bwd: null pointer");
  DX_REQUIRE(epilogue == 0 || epilogue == 1, "dx_disc_post_bwd: bad epilogue flag");
  DX_REQUIRE(!epilogue || (R && G), "dx_disc_post_bwd: null pointer (the epilogue needs R and G)");
  DX_REQUIRE(rows > 0 && rdiv > 0 && N > 0 && C > 0 && C % 4 == 0 && taps > 0 && taps % 2 == 1,
             "dx_disc_post_bwd: bad shape (positive sizes, C %% 4 == 0, odd taps)");
  DX_REQUIRE(sxn % 4 == 0 && sxr % 4 == 0 && sxb % 4 == 0 && dx_aligned16(dZ) && (!epilogue || (dx_aligned16(R) && dx_aligned16(G))),
             "dx_disc_post_bwd: the maps need strides %% 4 == 0 and 16-byte aligned pointers");
  const long total = (long)rows * N * (C / 4);
  DX_REQUIRE((total + THREADS - 1) / THREADS <= 0x7fffffffL, "dx_disc_post_bwd: too many outputs for one launch");
  hipLaunchKernelGGL(disc_post_bwd_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                     Sr, Sg, ssb, ssr, ssn, W, dZ, R, G, sxb, sxr, sxn, gw_gen, gw_fm, s_scale, fm_scale, rdiv, N, C, taps, epilogue, total);
  DX_LAUNCH_CHECK("dx_disc_post_bwd");
  return DX_OK;
}

int dx_disc_first_bwd(const float* dZ, const float* W, float* dy, long sdb, int T, int B, int p, int Cout, int taps, int stride, int pad,
                      int accumulate, void* stream) {
  DX_REQUIRE(dZ && W && dy, "dx_disc_first_bwd: null pointer");
  DX_REQUIRE(B > 0 && T > 0 && p > 0 && Cout > 0 && Cout % 4 == 0 && taps > 0 && stride > 0 && pad >= 0 && sdb >= T,
             "dx_disc_first_bwd: non-positive size (Cout %% 4 == 0, sdb >= T)");
  DX_REQUIRE(accumulate == 0 || accumulate == 1, "dx_disc_first_bwd: bad accumulate flag");
  DX_REQUIRE(T % p == 0 || p - T % p < T, "dx_disc_first_bwd: the reflect padding (p - T %% p samples) must be shorter than the signal");
  DX_REQUIRE(dx_aligned16(dZ), "dx_disc_first_bwd: dZ must be 16-byte aligned");
  const int H = dx_cdiv(T, p);
  DX_REQUIRE(H + 2 * pad >= taps, "dx_disc_first_bwd: unsupported shape (H + 2 pad >= taps)");
  const int Hout = (H + 2 * pad - taps) / stride + 1;
  const long total = (long)B * T;
  const long blocks = (total * SUB + THREADS - 1) / THREADS;
  DX_REQUIRE(blocks <= 0x7fffffffL, "dx_disc_first_bwd: too many samples for one launch");
  hipLaunchKernelGGL(disc_first_bwd_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream,
                     dZ, W, dy, sdb, T, p, H, Hout, Cout, taps, stride, pad, accumulate, total);
  DX_LAUNCH_CHECK("dx_disc_first_bwd");
  return DX_OK;
}

int dx_disc_pool_bwd(const float* dy, float* dx, int R, int T, int accumulate, void* stream) {
  DX_REQUIRE(dy && dx, "dx_disc_pool_bwd: null pointer");
  DX_REQUIRE(dy != dx, "dx_disc_pool_bwd: dx must not alias dy");
  DX_REQUIRE(R > 0 && T > 0, "dx_disc_pool_bwd: non-positive size");
  DX_REQUIRE(accumulate == 0 || accumulate == 1, "dx_disc_pool_bwd: bad accumulate flag");
  const long total = (long)R * T;
  DX_REQUIRE((total + THREADS - 1) / THREADS <= 0x7fffffffL, "dx_disc_pool_bwd: too many samples for one launch");
  hipLaunchKernelGGL(disc_pool_bwd_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                     dy, dx, T, T / 2 + 1, accumulate, total);
  DX_LAUNCH_CHECK("dx_disc_pool_bwd");
  return DX_OK;
}

}  // extern "C"
