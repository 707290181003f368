// Row-pass helpers shared by the LayerNorm kernels (dx_rows.hip) and the fused attention + out-projection + LayerNorm launch (dx_attention.hip).
// Included inside each file's anonymous namespace.  ln_fwd_kernel, proj_ln_fwd_kernel and attn_proj_ln_fwd_kernel run the SAME row arithmetic
// (ln_row_finish), the two fused launches the same tile step, prologue and out-projection: bit-equal outputs by construction.
#pragma once
// LDS pointers reach the shared helpers WITH their address space (the callers cast): a helper is optimised on its own before it is
// inlined, and from a generic pointer its LDS addressing comes out unlike that of a kernel that held the same code inline (offsets added
// again in every key tile instead of riding on the instruction).
typedef __attribute__((address_space(3))) unsigned char* lds_bytes;
typedef __attribute__((address_space(3))) float* lds_floats;
constexpr float LN_EPS = 1e-5f;

// Row layout in a wave: LPR lanes share one row and a wave walks 64/LPR rows at once.  C = 128 rows are only 512 bytes,
// so one row per wave-instruction leaves the memory pipe mostly idle; 16 lanes x two 16-byte accesses per row puts
// four rows (2 KB per tensor) in flight per wave.  C = 1024 keeps the whole wave on one row.
template <int C> struct RowVec {
  static constexpr int V = 4;                           // floats per access
  static constexpr int LPR = (C >= 256) ? 64 : 16;      // lanes per row
  static constexpr int RPW = 64 / LPR;                  // rows per wave
  static constexpr int K = C / (LPR * V);               // accesses per lane
  static constexpr int E = K * V;
  static_assert(C % (LPR * V) == 0, "C must be a multiple of 64");
};

// p = base of the lane's row, l = lane % LPR
template <int C>
__device__ __forceinline__ void row_load(const float* p, int l, float v[RowVec<C>::E]) {
#pragma unroll
  for (int k = 0; k < RowVec<C>::K; ++k) {
    const float4 t = *reinterpret_cast<const float4*>(p + (k * RowVec<C>::LPR + l) * 4);
    v[k * 4 + 0] = t.x; v[k * 4 + 1] = t.y; v[k * 4 + 2] = t.z; v[k * 4 + 3] = t.w;
  }
}
template <int C>
__device__ __forceinline__ void row_store(float* p, int l, const float v[RowVec<C>::E]) {
#pragma unroll
  for (int k = 0; k < RowVec<C>::K; ++k)
    *reinterpret_cast<float4*>(p + (k * RowVec<C>::LPR + l) * 4) = make_float4(v[k * 4], v[k * 4 + 1], v[k * 4 + 2], v[k * 4 + 3]);
}
// bf16-stored rows: same lane -> column map, 8-byte accesses
template <int C>
__device__ __forceinline__ void row_load(const dx_h16* p, int l, float v[RowVec<C>::E]) {
#pragma unroll
  for (int k = 0; k < RowVec<C>::K; ++k) {
    const bf16x4 t = *reinterpret_cast<const bf16x4*>(p + (k * RowVec<C>::LPR + l) * 4);
    v[k * 4 + 0] = (float)t[0]; v[k * 4 + 1] = (float)t[1]; v[k * 4 + 2] = (float)t[2]; v[k * 4 + 3] = (float)t[3];
  }
}
template <int C>
__device__ __forceinline__ void row_store(dx_h16* p, int l, const float v[RowVec<C>::E]) {
#pragma unroll
  for (int k = 0; k < RowVec<C>::K; ++k) {
    bf16x4 t;
    t[0] = (dx_h16)v[k * 4]; t[1] = (dx_h16)v[k * 4 + 1]; t[2] = (dx_h16)v[k * 4 + 2]; t[3] = (dx_h16)v[k * 4 + 3];
    *reinterpret_cast<bf16x4*>(p + (k * RowVec<C>::LPR + l) * 4) = t;
  }
}
template <int C> __device__ __forceinline__ int row_col(int l, int idx) {
  return ((idx / 4) * RowVec<C>::LPR + l) * 4 + (idx % 4);
}
// sum over the LPR lanes that share a row (every lane of the group gets the total)
template <int C> __device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int off = RowVec<C>::LPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// keep/scale factors of the lane's E elements of a row: its K groups of 4 consecutive channels are one 64-bit draw each (the same
// values dx_dropout_scale() gives element by element, at a quarter of the hashing)
template <int C>
__device__ __forceinline__ void row_dropout(uint64_t seed, uint64_t row, int l, uint32_t thresh, float inv_keep, float f[RowVec<C>::E]) {
#pragma unroll
  for (int k = 0; k < RowVec<C>::K; ++k) dx_dropout_scale4(seed, row * C + (uint64_t)((k * RowVec<C>::LPR + l) * 4), thresh, inv_keep, f + 4 * k);
}

// LayerNorm affine of the lane's E channels
template <int C>
__device__ __forceinline__ void row_affine(const float* w, const float* bias, int l, float (&wv)[RowVec<C>::E], float (&bv)[RowVec<C>::E]) {
#pragma unroll
  for (int e = 0; e < RowVec<C>::E; ++e) { wv[e] = w[row_col<C>(l, e)]; bv[e] = bias[row_col<C>(l, e)]; }
}

// Dropout on the LayerNorm output: thresh = 0 (a literal in the fused launches, so it folds away) = off.  f = the lane's factors of
// the current row: a kernel keeps ONE of these for all its rows (as a local of the row pass the compiler zeroes the E unused factors
// again for every row).
template <int C> struct RowPostDrop { uint64_t seed; uint32_t thresh; float inv_keep; float f[RowVec<C>::E]; };

// The LayerNorm row pass from the lane's z[E] on: mean, rstd, y = mask(film(drop_post(LN(z)))) and the stores of mean, rstd, y and the
// 16-bit copy of y.  Every lane of a row group runs the arithmetic (row_sum is cross-lane); a lane whose row is out of range (!inb) or
// padded (!valid) runs it on zeros.  IO = storage type of y.
template <int C, typename IO>
__device__ __forceinline__ void ln_row_finish(const float (&z)[RowVec<C>::E], bool inb, bool valid, long row, int b, int l,
                                              const float (&wv)[RowVec<C>::E], const float (&bv)[RowVec<C>::E], const float* film, int ld_film,
                                              RowPostDrop<C>& post, float* mean, float* rstd, IO* y_out, dx_h16* y_h) {
  constexpr int E = RowVec<C>::E;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) s += z[e];
  const float mu = row_sum<C>(s) * (1.0f / C);
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) { const float d = z[e] - mu; q += d * d; }
  const float rs = 1.0f / sqrtf(row_sum<C>(q) * (1.0f / C) + LN_EPS);
  // padded rows: the output is zero by definition and nothing reads z / mean / rstd of them (the backward skips them too)
  if (inb && l == 0) { mean[row] = valid ? mu : 0.f; rstd[row] = valid ? rs : 0.f; }
  float y[E];
  if (post.thresh) row_dropout<C>(post.seed, (uint64_t)row, l, post.thresh, post.inv_keep, post.f);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int c = row_col<C>(l, e);
    float t = (z[e] - mu) * rs * wv[e] + bv[e];
    if (post.thresh) t *= post.f[e];
    if (film) t = film[(size_t)b * ld_film + c] * t + film[(size_t)b * ld_film + C + c];
    y[e] = valid ? t : 0.f;
  }
  if (inb) {
    row_store<C>(y_out + row * C, l, y);
    if constexpr (sizeof(IO) == 4 && C < 256) { if (y_h) row_store<C>(y_h + row * C, l, y); }
  }
}

// ---- the pieces the fused launches share (proj_ln_fwd_kernel: 4 waves x 4 steps per 64-row tile, attn_proj_ln_fwd_kernel: 8 waves x 2 steps; C = 128) ----
// Everything the row pass needs from global memory is requested BEFORE the matrix phase (the residual rows of the lane's steps, the
// LayerNorm affine): a workgroup is one short dependent chain, and with these loads behind the barrier the 5.8 k-row symbol-level
// launch took 24 us for 3 MB.
template <int C, int STEPS> struct LnRowsAhead {
  static constexpr int E = RowVec<C>::E;
  bool valid[STEPS]; int b[STEPS]; long row[STEPS];     // row = -1: out of range
  float rv[STEPS][E], wv[E], bv[E];
  __device__ __forceinline__ void request(int st, bool inb, bool vld, int bb, long r, const float* res, int l) {
    valid[st] = vld; b[st] = bb; row[st] = inb ? r : -1;
#pragma unroll
    for (int e = 0; e < E; ++e) rv[st][e] = 0.f;
    if (vld && res) row_load<C>(res + r * C, l, rv[st]);
  }
};

// The 128-wide out-projection of a wave's 16 tokens: NB blocks of 16 output channels from block i0 (W = A operand from the fragment-major
// pack, X^T = B operand: xb = the four K-steps of token `tok`'s 16-bit row, a lane owns 4 channels of that token), K order 0..3, into
// the fp32 tile (4-float slots ^ (tok & 15)).
template <int NB>
__device__ __forceinline__ void proj128_to_tile(const bf16x8 (&xb)[4], const dx_h16* Wp, const float* proj_bias, int i0, int lane, int tok, lds_floats tile3) {
  float* const tile = (float*)tile3;
  const int g = lane >> 4;
  f32x4 acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i)
    acc[i] = proj_bias ? *reinterpret_cast<const f32x4*>(proj_bias + (i0 + i) * 16 + g * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    bf16x8 wa[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) wa[i] = *reinterpret_cast<const bf16x8*>(Wp + (size_t)((i0 + i) * 4 + ks) * 512 + lane * 8);
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = DX_MFMA_H16(wa[i], xb[ks], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < NB; ++i)
    *reinterpret_cast<f32x4*>(tile + tok * 128 + ((((i0 + i) * 4 + g) ^ (tok & 15)) << 2)) = acc[i];
}

// The row pass on the tile: ln_fwd_kernel<128> with the projection result read from LDS (4 rows per wave-instruction, 16 lanes x 2 float4
// per row), the wave's STEPS steps of four rows from tile row lrow0 unrolled.  z = drop_pre(tile row) + the prefetched residual, kept for
// the backward (zeros on padded rows).
template <int C, int STEPS>
__device__ __forceinline__ void ln_tile_pass(lds_floats tile3, int lrow0, int l, int sub, const LnRowsAhead<C, STEPS>& ah,
                                             uint64_t seed_pre, uint32_t thresh_pre, float inv_keep_pre, const float* film, int ld_film,
                                             float* z_out, float* mean, float* rstd, float* y, dx_h16* y_h) {
  constexpr int E = RowVec<C>::E, LPR = RowVec<C>::LPR;
  const float* const tile = (const float*)tile3;
  RowPostDrop<C> no_post{0, 0, 0.f};
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    const int lrow = lrow0 + st * 4 + sub;
    const long row = ah.row[st];
    const bool inb = row >= 0, vld = ah.valid[st];
    float z[E];
#pragma unroll
    for (int e = 0; e < E; ++e) z[e] = 0.f;
    if (vld) {
#pragma unroll
      for (int k = 0; k < RowVec<C>::K; ++k) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(tile + lrow * C + (((k * LPR + l) ^ (lrow & 15)) << 2));
        z[k * 4 + 0] = t[0]; z[k * 4 + 1] = t[1]; z[k * 4 + 2] = t[2]; z[k * 4 + 3] = t[3];
      }
      if (thresh_pre) {
        float f[E];
        row_dropout<C>(seed_pre, (uint64_t)row, l, thresh_pre, inv_keep_pre, f);
#pragma unroll
        for (int e = 0; e < E; ++e) z[e] *= f[e];
      }
#pragma unroll
      for (int e = 0; e < E; ++e) z[e] += ah.rv[st][e];
    }
    if (inb) row_store<C>(z_out + row * C, l, z);
    ln_row_finish<C, float>(z, inb, vld, row, ah.b[st], l, ah.wv, ah.bv, film, ld_film, no_post, mean, rstd, y, y_h);
  }
}
