// Mel front end (reference extract_features.py mel_spectrogram_HiFi, vocoder/dataset.py mel_spectrogram with center = False):
// waveform (B, S) -> log-mel (B, n_mels, T) and frame energy (B, T), one launch.
//
// One workgroup takes MF = 32 consecutive frames of ONE batch row.  It stages the MF * 256 + 768 padded samples those frames cover
// into LDS, applying the row's own reflect padding (384 samples each side) while staging; frame m is then the strided view
// [256 m, 256 m + 1024) of that window, in segments of 256 samples whose LDS stride (260 floats) spreads the 16 frames of an MFMA
// row block over the 64 banks.  The DFT is a GEMM [MF x 1024] . [1024 x 2 kmaxp] on v_mfma_f32_16x16x4_f32 (exact f32 products,
// f32 accumulation) against a basis with the periodic Hann window folded in (computed in double, rounded once to f32, packed as
// MFMA B fragments by dx_mel_pack, read from L2).  Each 16-sample K step is summed from zero and then added to the running sum, which
// keeps the rounding of the small leakage bins near that of torch's FFT.  The epilogue takes sqrt(re^2 + im^2 + 1e-9) into LDS, runs
// the [MF x kmaxp] . [kmaxp x n_mels] mel GEMM from there, clamps, takes the log and writes (B, n_mels, T) plus the L2 norm of the
// clamped mel over channels (the frame energy).
//
// Valid lengths.  lengths[b] samples of row b exist (samples past it are never read); the row has lengths[b] / 256 frames and
// everything at or past that frame is written as 0.  Tiles start at frame 0 of each row and every output is summed in a fixed
// order without atomics, so batch row b is bitwise what the same utterance computes alone.
#include "dx_common.h"

namespace {

constexpr int NFFT = 1024, HOP = 256, PADR = 384;   // n_fft = win, hop, reflect pad (n_fft - hop) / 2
constexpr int KSTEPS = NFFT / 16;                    // 16-sample K steps of the DFT GEMM
constexpr int MF = 32;                               // frames per workgroup (two MFMA row blocks)
constexpr int SEGW = HOP + 4;                        // LDS stride of one 256-sample segment of the padded window
constexpr int THREADS = 256;

struct MelArgs {
  const float* wav; long sxb; int S;
  const int* lengths;
  const uint4* basis; const uint4* fb;
  float* mel; long smb; float* energy;
  int T_max, n_mels, kmaxp;
  float clip;
};

__host__ __device__ inline int mel_lds_floats(int kmaxp, int n_mels) {
  const int win = (MF + 3) * SEGW, mag = MF * (kmaxp + 4);
  return (win > mag ? win : mag) + MF * (n_mels + 1);
}

// Stages the (MF + 3) * 256 padded samples from padded sample f0 * 256 on (f0 may be negative in the backward: nothing lies before the
// padded row), reflecting at the row's own ends: padded sample i is source sample q = i - 384.
__device__ __forceinline__ void stage_window(float* Wd, const float* x, int f0, int len) {
  for (int i = threadIdx.x; i < (MF + 3) * HOP; i += THREADS) {
    const int q = f0 * HOP + i - PADR;
    float v = 0.f;                                   // past the padded row: read by no valid frame
    if (q >= -PADR && q < len + PADR) v = x[q < 0 ? -q : (q >= len ? 2 * (len - 1) - q : q)];
    Wd[(i >> 8) * SEGW + (i & (HOP - 1))] = v;
  }
}

// DFT GEMM of the staged window: acc[i][c][mb] = frames (row block mb) x bins (block i of this wave; c = 0 cos, 1 sin).
// Bp: this wave's and lane's fragment (bin block i, cos / sin c, K step ks) at Bp[((i * 2 + c) * KSTEPS + ks) * 64].
template <int NKB>
__device__ __forceinline__ void dft_gemm(const float* Wd, const uint4* Bp, int r, int g, f32x4 (&acc)[NKB][2][2]) {
  uint4 bc[NKB][2], bn[NKB][2];
#pragma unroll
  for (int i = 0; i < NKB; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      acc[i][c][0] = acc[i][c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      bc[i][c] = Bp[(i * 2 + c) * KSTEPS * 64];
    }
  for (int ks = 0; ks < KSTEPS; ++ks) {
    const int kn = ks + 1 < KSTEPS ? ks + 1 : ks;    // prefetch of the next step (the last step reloads its own)
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) bn[i][c] = Bp[((i * 2 + c) * KSTEPS + kn) * 64];
    const int o = ks * 16 + 4 * g;
    f32x4 a[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) a[mb] = *reinterpret_cast<const f32x4*>(Wd + (mb * 16 + r + (o >> 8)) * SEGW + (o & (HOP - 1)));
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) acc[i][c][mb] += dx_mma_f32_k16(a[mb], __builtin_bit_cast(f32x4, bc[i][c]), f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) bc[i][c] = bn[i][c];
  }
}

// NKB: 16-bin blocks per wave (kmaxp = 64 NKB); wave w owns bin blocks w NKB .. w NKB + NKB - 1, cos and sin, both row blocks.
template <int NKB>
__global__ void __launch_bounds__(THREADS) mel_kernel(MelArgs p) {
  extern __shared__ __attribute__((aligned(16))) float mel_smem[];
  const int b = blockIdx.y, t0 = blockIdx.x * MF, n_mels = p.n_mels;
  const int len = min(p.lengths[b], p.S);
  const int T = len > PADR ? min(len / HOP, p.T_max) : 0;
  float* melb = p.mel + b * p.smb;
  float* en = p.energy + (long)b * p.T_max;
  if (t0 >= T) {                                     // no valid frame in this tile: zeros only
    for (int e = threadIdx.x; e < MF * n_mels; e += THREADS) {
      const int t = t0 + e % MF, n = e / MF;
      if (t < p.T_max) melb[(long)n * p.T_max + t] = 0.f;
    }
    if (threadIdx.x < MF && t0 + (int)threadIdx.x < p.T_max) en[t0 + threadIdx.x] = 0.f;
    return;
  }
  // ---- stage the reflect-padded window: padded sample t0 * 256 + i is source sample q = t0 * 256 + i - 384 ----
  float* Wd = mel_smem;
  stage_window(Wd, p.wav + b * p.sxb, t0, len);
  __syncthreads();
  // ---- DFT GEMM ----
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  f32x4 acc[NKB][2][2];
  dft_gemm<NKB>(Wd, p.basis + (long)w * NKB * 2 * KSTEPS * 64 + lane, r, g, acc);
  __syncthreads();                                   // every wave is done with the window: the magnitudes take its place
  // ---- magnitude: sqrt((re^2 + im^2) + 1e-9), as torch's spec.pow(2).sum(-1) + 1e-9 ----
  const int ldm = p.kmaxp + 4;
  float* Mg = mel_smem;
#pragma unroll
  for (int i = 0; i < NKB; ++i)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float re = acc[i][0][mb][e], im = acc[i][1][mb][e];
        const float s = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
        Mg[(mb * 16 + 4 * g + e) * ldm + (w * NKB + i) * 16 + r] = __fsqrt_rn(__fadd_rn(s, 1e-9f));
      }
  __syncthreads();
  // ---- mel GEMM [MF x kmaxp] . [kmaxp x n_mels], clamp, log; (row block, column block) pairs round-robin over the waves ----
  const int ldl = n_mels + 1, NB = n_mels / 16, KS2 = p.kmaxp / 16;
  float* Ls = mel_smem + (mel_lds_floats(p.kmaxp, n_mels) - MF * ldl);
  for (int q = w; q < 2 * NB; q += 4) {
    const int mb = q & 1, nb = q >> 1;
    f32x4 c = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* Fp = p.fb + (long)nb * KS2 * 64 + lane;
    const float* A = Mg + (mb * 16 + r) * ldm + 4 * g;
    for (int ks = 0; ks < KS2; ++ks) c = dx_mma_f32_k16(*reinterpret_cast<const f32x4*>(A + ks * 16), __builtin_bit_cast(f32x4, Fp[ks * 64]), c);
    const int n = nb * 16 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = mb * 16 + 4 * g + e, t = t0 + m;
      const float v = fmaxf(c[e], p.clip);
      Ls[m * ldl + n] = v;
      if (t < p.T_max) melb[(long)n * p.T_max + t] = t < T ? logf(v) : 0.f;
    }
  }
  __syncthreads();
  // ---- frame energy: L2 norm of the clamped mel over channels, in channel order ----
  if (threadIdx.x < MF) {
    const int m = threadIdx.x, t = t0 + m;
    if (t < p.T_max) {
      float s = 0.f;
      for (int n = 0; n < n_mels; ++n) s = __builtin_fmaf(Ls[m * ldl + n], Ls[m * ldl + n], s);
      en[t] = t < T ? __fsqrt_rn(s) : 0.f;
    }
  }
}

// ---- backward: dwav = d(sum gmel . mel) / d(wav) -----------------------------------------------------------------------------------
// The forward saves nothing, so a workgroup recomputes re / im, the magnitudes and the linear mel of its frames exactly as mel_kernel
// does, then runs the chain backwards: dlin = gmel / lin where lin >= clip, dmag = dlin . fb (fb packed with bins as columns),
// dre = dmag re / mag, dim = dmag im / mag, dframe = [dre | dim] . basis^T (the basis packed with samples as columns), overlap-add,
// reflect fold, store.
//
// Ownership.  The padded row has T + 3 segments of 256 samples with a gradient; segment s takes frames s - 3 .. s.  A workgroup owns
// up to MF - 3 = 29 consecutive segments [sa, se) and computes the frames sa - 3 .. se - 1 (at most 32), so every owned segment is
// complete inside the workgroup: three halo frames per tile, on one side only, no workspace and no second pass.  The 384 reflected
// samples of the head land on source samples 1 .. 384 (padded 385 .. 768, segments 1 .. 3) and those of the tail on padded samples from
// len - 1 on (segments T - 1 .. T + 2), so the first tile must own segments 0 .. 3 and the last tile the last four: when the
// remainder of (T + 3) / 29 is 1 .. 3 the last boundary moves back to T - 1.  Each dwav element is then one workgroup's
// ((segment sum) + head mirror) + tail mirror, with the segment sum taken in frame order: no atomics, nothing depends on scheduling.
constexpr int OWN = MF - 3;                          // segments owned per workgroup
constexpr int DCH = 128, LDD = DCH + 4;              // K columns of one [dre | dim] chunk in LDS (4 waves x (16 cos + 16 sin)), its stride

struct MelBwdArgs {
  const float* wav; long sxb; int S;
  const int* lengths;
  const uint4* basis; const uint4* fb; const uint4* basisT; const uint4* fbT;
  const float* gmel; long sgb; float* dwav;
  int T_max, n_mels, kmaxp;
  float clip;
};

__host__ __device__ inline int mel_bwd_lds_floats(int kmaxp, int n_mels) {
  const int win = (MF + 3) * SEGW, mag = MF * (kmaxp + 4);        // window / overlap-add buffer (and two chunk buffers), magnitudes
  return (win > mag ? win : mag) + MF * (n_mels + 4);
}
static_assert(2 * MF * LDD <= (MF + 3) * SEGW, "the two [dre | dim] chunk buffers must fit in the window's place");

template <int NKB>
__global__ void __launch_bounds__(THREADS) mel_bwd_kernel(MelBwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float mel_smem[];
  const int b = blockIdx.y, j = blockIdx.x, n_mels = p.n_mels;
  const int len = min(p.lengths[b], p.S);
  const int T = len > PADR ? min(len / HOP, p.T_max) : 0;
  const int NS = T + 3;                              // padded segments that carry a gradient
  float* dx = p.dwav + b * p.sxb;
  {                                                  // zeros at and past the row's end (and past the last frame's reach, if T_max cuts the row short)
    const int zs = T > 0 ? min(len, NS * HOP - PADR) : 0;
    const int lo = max(zs, j * OWN * HOP - PADR), hi = j + 1 == (int)gridDim.x ? p.S : min(p.S, (j + 1) * OWN * HOP - PADR);
    for (int q = lo + threadIdx.x; q < hi; q += THREADS) dx[q] = 0.f;
  }
  const int nt = (NS + OWN - 1) / OWN;
  if (T == 0 || j >= nt) return;
  int sa = j * OWN, se = min(sa + OWN, NS);
  if (nt >= 2 && NS - OWN * (nt - 1) < 4) {          // keep the last four segments (the tail's mirror pairs) in one tile
    if (j == nt - 2) se = NS - 4;
    if (j == nt - 1) sa = NS - 4;
  }
  const int f0 = sa - 3, fend = min(T, se);          // local frame m is frame f0 + m, computed if 0 <= f0 + m < fend
  // ---- forward recompute: window, DFT GEMM, magnitudes (as mel_kernel) ----
  float* Wd = mel_smem;
  stage_window(Wd, p.wav + b * p.sxb, f0, len);
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  f32x4 acc[NKB][2][2];
  dft_gemm<NKB>(Wd, p.basis + (long)w * NKB * 2 * KSTEPS * 64 + lane, r, g, acc);
  __syncthreads();
  const int ldm = p.kmaxp + 4;
  float* Mg = mel_smem;
#pragma unroll
  for (int i = 0; i < NKB; ++i)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float re = acc[i][0][mb][e], im = acc[i][1][mb][e];
        const float s = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
        Mg[(mb * 16 + 4 * g + e) * ldm + (w * NKB + i) * 16 + r] = __fsqrt_rn(__fadd_rn(s, 1e-9f));
      }
  __syncthreads();
  // ---- lin = mag . fb^T as mel_kernel; dlin = gmel / lin where the clamp passes (lin >= clip), 0 for frames not computed ----
  const int ldl = n_mels + 4, NB = n_mels / 16, KS2 = p.kmaxp / 16;
  float* Dl = mel_smem + (mel_bwd_lds_floats(p.kmaxp, n_mels) - MF * ldl);
  const float* gb = p.gmel + b * p.sgb;
  for (int q = w; q < 2 * NB; q += 4) {
    const int mb = q & 1, nb = q >> 1;
    f32x4 c = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* Fp = p.fb + (long)nb * KS2 * 64 + lane;
    const float* A = Mg + (mb * 16 + r) * ldm + 4 * g;
    for (int ks = 0; ks < KS2; ++ks) c = dx_mma_f32_k16(*reinterpret_cast<const f32x4*>(A + ks * 16), __builtin_bit_cast(f32x4, Fp[ks * 64]), c);
    const int n = nb * 16 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = mb * 16 + 4 * g + e, t = f0 + m;
      float d = 0.f;
      if (t >= 0 && t < fend && c[e] >= p.clip) d = gb[(long)n * p.T_max + t] / c[e];
      Dl[m * ldl + n] = d;
    }
  }
  __syncthreads();                                   // dlin complete; the magnitudes are dead from here
  // ---- dmag = dlin . fb for this wave's own bins (the layout of acc), then dre = dmag re / mag, dim = dmag im / mag in place ----
#pragma unroll
  for (int i = 0; i < NKB; ++i) {
    f32x4 c[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const uint4* Fp = p.fbT + (long)(w * NKB + i) * NB * 64 + lane;
    for (int ks = 0; ks < NB; ++ks) {
      const f32x4 f = __builtin_bit_cast(f32x4, Fp[ks * 64]);
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) c[mb] = dx_mma_f32_k16(*reinterpret_cast<const f32x4*>(Dl + (mb * 16 + r) * ldl + ks * 16 + 4 * g), f, c[mb]);
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float re = acc[i][0][mb][e], im = acc[i][1][mb][e];
        const float s = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
        const float u = c[mb][e] / __fsqrt_rn(__fadd_rn(s, 1e-9f));
        acc[i][0][mb][e] = u * re;
        acc[i][1][mb][e] = u * im;
      }
  }
  // ---- dframe = [dre | dim] . basis^T: wave w takes samples [256 w, 256 w + 256) of every frame; K runs over the bins in NKB chunks
  // of 128 columns (bin block i of each wave, cos then sin), handed over through two LDS buffers; each 16-column K step is summed
  // from zero and then added, as in the forward ----
  f32x4 out[16][2];
#pragma unroll
  for (int cb = 0; cb < 16; ++cb) out[cb][0] = out[cb][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NKB; ++i) {
    float* D = mel_smem + (i & 1) * MF * LDD;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int e = 0; e < 4; ++e) D[(mb * 16 + 4 * g + e) * LDD + w * 32 + c * 16 + r] = acc[i][c][mb][e];
    __syncthreads();                                 // one barrier per chunk: the buffer written next was last read two chunks ago
    const uint4* Tp = p.basisT + ((long)(w * 16) * NKB + i) * (DCH / 16) * 64 + lane;   // fragment (column block, chunk, K step)
    for (int ks = 0; ks < DCH / 16; ++ks) {
      f32x4 a[2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) a[mb] = *reinterpret_cast<const f32x4*>(D + (mb * 16 + r) * LDD + ks * 16 + 4 * g);
#pragma unroll
      for (int cb = 0; cb < 16; ++cb) {
        const f32x4 t4 = __builtin_bit_cast(f32x4, Tp[((long)cb * NKB * (DCH / 16) + ks) * 64]);
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) out[cb][mb] += dx_mma_f32_k16(a[mb], t4, f32x4{0.f, 0.f, 0.f, 0.f});
      }
    }
  }
  __syncthreads();                                   // every wave is done with the chunk buffers: the overlap-add buffer takes their place
  // ---- overlap-add: segment m + w of the tile takes frame m's samples [256 w, 256 w + 256), added in the order w = 0, 1, 2, 3 ----
  float* O = mel_smem;
#pragma unroll 1
  for (int ww = 0; ww < 4; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int cb = 0; cb < 16; ++cb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float* o = O + (mb * 16 + 4 * g + e + w) * SEGW + cb * 16 + r;
            *o = ww == 0 ? out[cb][mb][e] : *o + out[cb][mb][e];
          }
    } else if (ww == 0) {                            // segments 32 .. 34 start from zero
      for (int i = threadIdx.x - 64; i < 3 * HOP; i += THREADS - 64) O[(MF + (i >> 8)) * SEGW + (i & (HOP - 1))] = 0.f;
    }
    __syncthreads();
  }
  // ---- fold the reflected ends onto the samples they mirror and store the owned samples ----
  for (int i = threadIdx.x; i < (se - sa) * HOP; i += THREADS) {
    const int pp = sa * HOP + i, q = pp - PADR;
    if (q < 0 || q >= len) continue;
    const int base = f0 * HOP;
    int l = pp - base;
    float v = O[(l >> 8) * SEGW + (l & (HOP - 1))];
    if (q >= 1 && q <= PADR) {                       // head: padded sample 384 - q is a copy of sample q
      l = PADR - q - base;
      v += O[(l >> 8) * SEGW + (l & (HOP - 1))];
    }
    const int ps = 2 * (len - 1) - q + PADR;         // tail: padded sample ps is a copy of sample q
    if (q >= len - 1 - PADR && q <= len - 2 && ps < NS * HOP) {
      l = ps - base;
      v += O[(l >> 8) * SEGW + (l & (HOP - 1))];
    }
    dx[q] = v;
  }
}

// Basis: [kb][c][ks][lane][4]: lane (n = l & 15, g = l >> 4) element v holds sample k = 16 ks + 4 g + v of bin 16 kb + n,
// hann(k) cos(2 pi bin k / 1024) for c = 0 and hann(k) sin(...) for c = 1, in double, rounded once.  Filter bank: [nb][ks][lane][4],
// element v of lane l holds fb[16 nb + (l & 15)][16 ks + 4 (l >> 4) + v] (0 past n_freq).
__global__ void mel_pack_kernel(const float* fb, int n_freq, int KS2, float* basis, float* fbp, long nbasis, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const double two_pi = 6.283185307179586476925287;
  if (e < nbasis) {
    const int v = (int)(e & 3), l = (int)((e >> 2) & 63), ks = (int)((e >> 8) & (KSTEPS - 1)), cb = (int)(e >> 14);
    const int k = ks * 16 + (l >> 4) * 4 + v, bin = (cb >> 1) * 16 + (l & 15);
    const double hann = 0.5 - 0.5 * cos(two_pi * k / NFFT);
    const double ph = two_pi * ((bin * k) & (NFFT - 1)) / NFFT;
    basis[e] = (float)(hann * ((cb & 1) ? sin(ph) : cos(ph)));
  } else {
    const long f = e - nbasis;
    const int v = (int)(f & 3), l = (int)((f >> 2) & 63), ks = (int)((f >> 8) % KS2), nb = (int)((f >> 8) / KS2);
    const int k = ks * 16 + (l >> 4) * 4 + v, n = nb * 16 + (l & 15);
    fbp[f] = k < n_freq ? fb[(long)n * n_freq + k] : 0.f;
  }
}

// Transposed operands of the backward.  basisT: [cb][i][ks][lane][4]: lane (n = l & 15, g = l >> 4) element v holds sample 16 cb + n of
// K column kk = 16 ks + 4 g + v of chunk i, which is bin 16 ((kk >> 5) NKB + i) + (kk & 15), cos for (kk >> 4) & 1 == 0 and sin for 1
// (the order mel_bwd_kernel lays its [dre | dim] chunks out in); the values are those of the forward basis.  fbT: [kb][ks][lane][4],
// element v of lane l holds fb[16 ks + 4 (l >> 4) + v][16 kb + (l & 15)] (0 past n_freq).
__global__ void mel_bwd_pack_kernel(const float* fb, int n_freq, int NKB, int NB, float* basisT, float* fbT, long nbasis, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const double two_pi = 6.283185307179586476925287;
  if (e < nbasis) {
    const int v = (int)(e & 3), l = (int)((e >> 2) & 63), ks = (int)((e >> 8) & (DCH / 16 - 1)), ci = (int)(e >> 11);
    const int i = ci % NKB, cb = ci / NKB, kk = ks * 16 + (l >> 4) * 4 + v;
    const int k = cb * 16 + (l & 15), bin = ((kk >> 5) * NKB + i) * 16 + (kk & 15);
    const double hann = 0.5 - 0.5 * cos(two_pi * k / NFFT);
    const double ph = two_pi * ((bin * k) & (NFFT - 1)) / NFFT;
    basisT[e] = (float)(hann * (((kk >> 4) & 1) ? sin(ph) : cos(ph)));
  } else {
    const long f = e - nbasis;
    const int v = (int)(f & 3), l = (int)((f >> 2) & 63), ks = (int)((f >> 8) % NB), kb = (int)((f >> 8) / NB);
    const int n = ks * 16 + (l >> 4) * 4 + v, bin = kb * 16 + (l & 15);
    fbT[f] = bin < n_freq ? fb[(long)n * n_freq + bin] : 0.f;
  }
}

template <int NKB>
int launch_mel(const MelArgs& a, int B, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&mel_kernel<NKB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)(mel_lds_floats(64 * NKB, 128) * sizeof(float)));
    configured = true;
  }
  const size_t smem = (size_t)mel_lds_floats(a.kmaxp, a.n_mels) * sizeof(float);
  hipLaunchKernelGGL(mel_kernel<NKB>, dim3(dx_cdiv(a.T_max, MF), B), dim3(THREADS), smem, s, a);
  DX_LAUNCH_CHECK("dx_mel");
  return DX_OK;
}

template <int NKB>
int launch_mel_bwd(const MelBwdArgs& a, int B, hipStream_t s) {
  static bool configured = false;
  if (!configured) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&mel_bwd_kernel<NKB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)(mel_bwd_lds_floats(64 * NKB, 128) * sizeof(float)));
    configured = true;
  }
  const size_t smem = (size_t)mel_bwd_lds_floats(a.kmaxp, a.n_mels) * sizeof(float);
  const int segs = (a.T_max > a.S / HOP ? a.T_max : a.S / HOP) + 4;   // the tiles' nominal sample ranges reach past S: they write the zeros
  hipLaunchKernelGGL(mel_bwd_kernel<NKB>, dim3(dx_cdiv(segs, OWN), B), dim3(THREADS), smem, s, a);
  DX_LAUNCH_CHECK("dx_mel_bwd");
  return DX_OK;
}

bool mel_shape_ok(int n_mels, int kmax) { return n_mels > 0 && n_mels % 16 == 0 && n_mels <= 128 && kmax > 0 && kmax <= NFFT / 2; }

}  // namespace

extern "C" {

int dx_mel_basis_size(int n_mels, int kmax, long* basis_bytes, long* fb_bytes) {
  DX_REQUIRE(basis_bytes && fb_bytes, "dx_mel_basis_size: null output");
  DX_REQUIRE(mel_shape_ok(n_mels, kmax), "dx_mel_basis_size: bad shape (n_mels %% 16 == 0 and <= 128, 0 < kmax <= 512)");
  const long kmaxp = dx_roundup(kmax, 64);
  *basis_bytes = kmaxp * 2 * NFFT * 4;
  *fb_bytes = (long)n_mels * kmaxp * 4;
  return DX_OK;
}

int dx_mel_pack(const float* fb, int n_mels, int n_freq, int kmax, void* basis, void* fbp, void* stream) {
  DX_REQUIRE(fb && basis && fbp, "dx_mel_pack: null pointer");
  DX_REQUIRE(mel_shape_ok(n_mels, kmax) && n_freq >= kmax,
             "dx_mel_pack: bad shape (n_mels %% 16 == 0 and <= 128, 0 < kmax <= min(512, n_freq))");
  const int kmaxp = dx_roundup(kmax, 64);
  const long nbasis = (long)kmaxp * 2 * NFFT, total = nbasis + (long)n_mels * kmaxp;
  hipLaunchKernelGGL(mel_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     fb, n_freq, kmaxp / 16, (float*)basis, (float*)fbp, nbasis, total);
  DX_LAUNCH_CHECK("dx_mel_pack");
  return DX_OK;
}

int dx_mel(const float* wav, long sxb, int S, const int* lengths, const void* basis, const void* fb, float* mel, long smb,
           float* energy, int B, int T_max, int n_mels, int kmax, float clip, void* stream) {
  DX_REQUIRE(wav && lengths && basis && fb && mel && energy, "dx_mel: null pointer");
  DX_REQUIRE(B > 0 && T_max > 0 && S > 0 && sxb >= S && smb >= (long)n_mels * T_max && mel_shape_ok(n_mels, kmax),
             "dx_mel: bad shape (sxb >= S, smb >= n_mels T_max; n_mels %% 16 == 0 and <= 128, 0 < kmax <= 512)");
  MelArgs a;
  a.wav = wav; a.sxb = sxb; a.S = S; a.lengths = lengths;
  a.basis = reinterpret_cast<const uint4*>(basis); a.fb = reinterpret_cast<const uint4*>(fb);
  a.mel = mel; a.smb = smb; a.energy = energy;
  a.T_max = T_max; a.n_mels = n_mels; a.kmaxp = dx_roundup(kmax, 64); a.clip = clip;
  hipStream_t s = (hipStream_t)stream;
  switch (a.kmaxp / 64) {
    case 1: return launch_mel<1>(a, B, s);
    case 2: return launch_mel<2>(a, B, s);
    case 3: return launch_mel<3>(a, B, s);
    case 4: return launch_mel<4>(a, B, s);
    case 5: return launch_mel<5>(a, B, s);
    case 6: return launch_mel<6>(a, B, s);
    case 7: return launch_mel<7>(a, B, s);
    default: return launch_mel<8>(a, B, s);
  }
}

int dx_mel_bwd_pack(const float* fb, int n_mels, int n_freq, int kmax, void* basisT, void* fbT, void* stream) {
  DX_REQUIRE(fb && basisT && fbT, "dx_mel_bwd_pack: null pointer");
  DX_REQUIRE(mel_shape_ok(n_mels, kmax) && n_freq >= kmax,
             "dx_mel_bwd_pack: bad shape (n_mels %% 16 == 0 and <= 128, 0 < kmax <= min(512, n_freq))");
  const int kmaxp = dx_roundup(kmax, 64);
  const long nbasis = (long)kmaxp * 2 * NFFT, total = nbasis + (long)n_mels * kmaxp;
  hipLaunchKernelGGL(mel_bwd_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     fb, n_freq, kmaxp / 64, n_mels / 16, (float*)basisT, (float*)fbT, nbasis, total);
  DX_LAUNCH_CHECK("dx_mel_bwd_pack");
  return DX_OK;
}

int dx_mel_bwd(const float* wav, long sxb, int S, const int* lengths, const void* basis, const void* fb, const void* basisT,
               const void* fbT, const float* gmel, long sgb, float* dwav, int B, int T_max, int n_mels, int kmax, float clip,
               void* stream) {
  DX_REQUIRE(wav && lengths && basis && fb && basisT && fbT && gmel && dwav, "dx_mel_bwd: null pointer");
  DX_REQUIRE(dwav != wav, "dx_mel_bwd: dwav must not alias wav");
  DX_REQUIRE(B > 0 && T_max > 0 && S > 0 && sxb >= S && sgb >= (long)n_mels * T_max && mel_shape_ok(n_mels, kmax),
             "dx_mel_bwd: bad shape (sxb >= S, sgb >= n_mels T_max; n_mels %% 16 == 0 and <= 128, 0 < kmax <= 512)");
  MelBwdArgs a;
  a.wav = wav; a.sxb = sxb; a.S = S; a.lengths = lengths;
  a.basis = reinterpret_cast<const uint4*>(basis); a.fb = reinterpret_cast<const uint4*>(fb);
  a.basisT = reinterpret_cast<const uint4*>(basisT); a.fbT = reinterpret_cast<const uint4*>(fbT);
  a.gmel = gmel; a.sgb = sgb; a.dwav = dwav;
  a.T_max = T_max; a.n_mels = n_mels; a.kmaxp = dx_roundup(kmax, 64); a.clip = clip;
  hipStream_t s = (hipStream_t)stream;
  switch (a.kmaxp / 64) {
    case 1: return launch_mel_bwd<1>(a, B, s);
    case 2: return launch_mel_bwd<2>(a, B, s);
    case 3: return launch_mel_bwd<3>(a, B, s);
    case 4: return launch_mel_bwd<4>(a, B, s);
    case 5: return launch_mel_bwd<5>(a, B, s);
    case 6: return launch_mel_bwd<6>(a, B, s);
    case 7: return launch_mel_bwd<7>(a, B, s);
    default: return launch_mel_bwd<8>(a, B, s);
  }
}

}  // extern "C"
