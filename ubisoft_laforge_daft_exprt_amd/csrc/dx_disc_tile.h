// What the discriminators' implicit-GEMM convolution (dx_disc.hip: dx_disc_conv) and its data gradient (dx_disc_bwd.hip:
// dx_disc_conv_dgrad) share: a tile of DT positions of ONE row times 64 * NI channels, 4 waves, wave w owning the 16-wide column blocks
// w + 4 i; a window of the input staged in LDS one chunk of reduction channels at a time; the weights read fragment by fragment from
// a pack laid out [...][column block][chunk][k step][lane][VEC]; and the blocked K sum.  Private to those two files.
#pragma once
#include "dx_common.h"

namespace {

constexpr float DISC_SLOPE = 0.1f;
constexpr int DT = 64;              // positions per tile (4 MFMA row blocks)
constexpr int THREADS = 256;
// k steps per block of the K sum (64 products in either mode): the discriminators' rule, see disc_chunk_mma
template <bool BF> constexpr int DISC_BLOCK = BF ? 16 : 4;

// Row `row` of a buffer addressed by (batch stride, column stride): batch row row / rdiv, column row % rdiv of the period-folded tensor.
__device__ __forceinline__ long disc_row_offset(int row, int rdiv, long sb, long sr) {
  const int rb = row / rdiv, rc = row - rb * rdiv;
  return rb * sb + rc * sr;
}

// A[lrow(rr)][cc] = X[(n0 + rr) * sn + cc] for rr < rows, cc < 4 * q4; zero where position n0 + rr is outside [0, N).
template <bool BF, typename RowMap>
__device__ __forceinline__ void disc_stage(typename DxMmaOp<BF>::T* A, int lda, const float* X, long sn, int n0, int N, int rows, int q4,
                                           RowMap lrow) {
  typedef DxMmaOp<BF> Op;
  for (int e = threadIdx.x; e < rows * q4; e += THREADS) {
    const int rr = e / q4, cc = (e - rr * q4) * 4, n = n0 + rr;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n >= 0 && n < N) v = *reinterpret_cast<const float4*>(X + (long)n * sn + cc);
    typename Op::T* d = A + lrow(rr) * lda + cc;
    d[0] = Op::cvt(v.x); d[1] = Op::cvt(v.y); d[2] = Op::cvt(v.z); d[3] = Op::cvt(v.w);
  }
}

// One chunk of the K sum: k = t * (cmask + 1) + c, k group t (a tap) at LDS rows lrow(t) + 0..63, channel c at column coff + c.
// Wp points at this wave's first column block and this chunk; wstride is the distance to its next column block, in fragments.
// The K sum is blocked: DISC_BLOCK k steps of one chunk (64 products in f32) run as one MFMA chain from zero in `part`, and the block
// sums are added into `acc` in order; the caller's epilogue adds the last one (acc + part).  One chain over a 5120-product sum loses
// about four times as much to rounding, which costs the scores the parity rule's mean bar.  The caller declares both zero-initialised
// (`f32x4 acc[NI][4] = {}, part[NI][4] = {}`): a helper that zeroes them through references costs the NI = 2 and 4 kernels an
// occupancy tier (the accumulators of both end up in AGPRs).
template <bool BF, int NI, typename RowMap>
__device__ __forceinline__ void disc_chunk_mma(const typename DxMmaOp<BF>::T* A, int lda, int coff, const uint4* Wp, long wstride, int KST,
                                               int K, int lg, int cmask, RowMap lrow, f32x4 (&acc)[NI][4], f32x4 (&part)[NI][4]) {
  typedef DxMmaOp<BF> Op;
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  for (int ks = 0; ks < KST; ++ks) {
    if ((ks & (DISC_BLOCK<BF> - 1)) == 0) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] += part[i][j];
          part[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const int k0 = ks * Op::KS + g * Op::VEC;
    const bool valid = k0 < K;                                         // past K the pack holds zeros; A must not be read there
    const int t = valid ? k0 >> lg : 0, c = k0 & cmask;
    const typename Op::T* ap = A + (lrow(t) + r) * lda + coff + c;
    uint4 b[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) b[i] = Wp[i * wstride + (long)ks * 64 + lane];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint4 a = make_uint4(0u, 0u, 0u, 0u);
      if (valid) a = *reinterpret_cast<const uint4*>(ap + j * 16 * lda);
#pragma unroll
      for (int i = 0; i < NI; ++i) part[i][j] = Op::mma(a, b[i], part[i][j]);
    }
  }
}

// Element e of a [...][column block][chunk][k step][lane][VEC] pack.  disc_pack_lane: f = its [...][k step] index, k = the lane's
// k inside the step (lane l element v: (l >> 4) * VEC + v), n = l & 15.  disc_pack_step, once f counts inside one [column block][chunk]
// [k step] array: k and n become the k inside the chunk and the channel nb * 16 + n.
struct DiscPackIdx { long f; int k, n, ch, nb; };
template <bool BF>
__device__ __forceinline__ DiscPackIdx disc_pack_lane(long e) {
  typedef DxMmaOp<BF> Op;
  const int v = (int)(e % Op::VEC), lane = (int)(e / Op::VEC % 64);
  DiscPackIdx x;
  x.f = e / Op::VEC / 64; x.k = (lane >> 4) * Op::VEC + v; x.n = lane & 15;
  return x;
}
template <bool BF>
__device__ __forceinline__ void disc_pack_step(DiscPackIdx& x, int KST, int nchunks) {
  x.k += (int)(x.f % KST) * DxMmaOp<BF>::KS; x.f /= KST;
  x.ch = (int)(x.f % nchunks);
  x.nb = (int)(x.f / nchunks);
  x.n += x.nb * 16;
}

}  // namespace
