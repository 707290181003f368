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

__device__ __forceinline__ f32x4 mma4(const f32x4& a, const uint4& b4, f32x4 c) {
  const f32x4 b = __builtin_bit_cast(f32x4, b4);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
  return c;
}

__host__ __device__ inline int mel_lds_floats(int kmaxp, int n_mels) {
  const int win = (MF + 3) * SEGW, mag = MF * (kmaxp + 4);
  return (win > mag ? win : mag) + MF * (n_mels + 1);
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
  const float* x = p.wav + b * p.sxb;
  for (int i = threadIdx.x; i < (MF + 3) * HOP; i += THREADS) {
    const int q = t0 * HOP + i - PADR;
    float v = 0.f;                                   // past the padded row: read by no valid frame
    if (q < len + PADR) v = x[q < 0 ? -q : (q >= len ? 2 * (len - 1) - q : q)];
    Wd[(i >> 8) * SEGW + (i & (HOP - 1))] = v;
  }
  __syncthreads();
  // ---- DFT GEMM ----
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const uint4* Bp = p.basis + (long)w * NKB * 2 * KSTEPS * 64 + lane;   // fragment (bin block i, cos / sin c, K step ks)
  f32x4 acc[NKB][2][2];
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
        for (int mb = 0; mb < 2; ++mb) acc[i][c][mb] += mma4(a[mb], bc[i][c], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
    for (int i = 0; i < NKB; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) bc[i][c] = bn[i][c];
  }
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
    for (int ks = 0; ks < KS2; ++ks) c = mma4(*reinterpret_cast<const f32x4*>(A + ks * 16), Fp[ks * 64], c);
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

}  // extern "C"
