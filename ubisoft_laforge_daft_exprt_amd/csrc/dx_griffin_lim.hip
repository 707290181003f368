// Griffin-Lim on the device (reference griffin_lim.py:100-198): mel -> linear magnitudes by non-negative least squares, the phase
// iteration, and the peak normalisation.  fp32 throughout; one geometry, n_fft = win = 1024 and hop = 256.
//
// dx_gl_iter: one iteration x_in -> x_out for a padded batch, one launch.  Row b has T = frames[b] frames and 256 T + 1024 samples,
// i.e. T + 4 hop blocks of 256; block s takes the frames s - 3 .. s that exist, so blocks 0 .. T + 2 carry signal and block T + 3 is 0
// after any iteration.  A workgroup of 8 waves owns GL_OWN = 13 consecutive blocks of one row and transforms the 16 frames
// f0 = 13 j - 3 .. f0 + 15 that touch them (the three on the left are recomputed, not communicated).  Wave w takes the frames
// f0 + 2 w and f0 + 2 w + 1 as ONE complex transform z = hann . (x_a + i x_b):
//   analysis   Z = FFT(z);  2 A[k] = Z[k] + conj(Z[-k]),  2 B[k] = (Z[k] - conj(Z[-k])) / i  (DC and Nyquist come out purely real)
//   projection P = M . S / |S|, (M, 0) where re^2 + im^2 == 0 (the factor 2 is left in S: the projection does not see it)
//   synthesis  Y[k] = P_A[k] + i P_B[k], Y[-k] = conj(P_A[k]) + i conj(P_B[k]); y_a + i y_b = IFFT(Y), run as the SAME forward
//              transform on (im, re) swapped, read back swapped; 1 / 1024 is folded into the final scale
// The transform is a Stockham radix-4 FFT, passes Ns = 1, 4, 16, 64, 256 on the wave's own 1024 complex points in LDS, re and im as
// separate float arrays.  In pass Ns lane l does the butterflies j = l + 64 c, c = 0 .. 3: it takes points j + 256 r, multiplies by the
// pass's twiddles (a table laid out per pass as [r - 1][j mod Ns], so the lanes read it contiguously) and produces points
// (j / Ns) 4 Ns + j mod Ns + r Ns.  The 16 outputs of a lane in pass 1 (and 16) are exactly the inputs of four butterflies of pass 4
// (and 64), so those pairs of passes run in registers: three trips through LDS per transform, not five.  Point i lives at float
// i + (i >> 4): with that skew the strided writes (lane stride 16 after the first pair, runs of 16 lanes 256 apart after the second)
// fall on distinct banks, and the stride-1 reads stay 2-way at worst.  All 16 reads of a lane come before a barrier, all 16 writes
// after it, so a trip works in place (the last pass reads and writes the same points and needs none in between).  Twiddles and the
// symmetric Hann window come from a host table computed in double and rounded once (no device sin / cos).
// The overlap-add sums the up-to-four contributions hann[n] y_f[n] of an output sample in frame order from the waves' LDS buffers,
// scales by 1 / 2048 (1 / n_fft of the inverse transform and the reference's / (n_fft / hop / 2)) and stores the owned blocks once:
// no atomics, no workspace, every sum in a fixed order, and tiles start at block 0 of each row, so a batch row is bitwise the
// utterance alone.  Blocks at or past T + 3 are written as 0; x_in and mag are never read past a row's own samples / frames.
//
// dx_nnls_mel: per frame, x0 = max(pinv(A) m, 0), then a fixed number of FISTA steps on 1/2 |A x - m|^2, x >= 0, with step
// 1 / |A|_2^2.  One wave per frame, lane l holds bins l + 64 i.  A is used in two packed forms: per channel (its contiguous run of
// non-zero weights) for A y, per bin (the at most two channels that weigh it) for A^T r.
#include "dx_common.h"

namespace {

constexpr int NFFT = 1024, HOP = 256, NBINS = NFFT / 2 + 1;
constexpr int GL_WAVES = 8, GL_THREADS = 64 * GL_WAVES;
constexpr int GL_FRAMES = 2 * GL_WAVES;               // frames a workgroup transforms
constexpr int GL_OWN = GL_FRAMES - 3;                 // hop blocks it owns
constexpr int FSTR = NFFT + NFFT / 16;                // floats of one skewed 1024-point array
constexpr int GL_LDS_FLOATS = 2 * NFFT + GL_WAVES * 2 * FSTR;
// host table (3072 floats): [0, 1024) symmetric Hann; [1024, 2048) twiddle cos, [2048, 3072) twiddle -sin, pass Ns at offset Ns - 4
// as [r - 1][q]

__device__ __forceinline__ int skew(int i) { return i + (i >> 4); }

struct GlArgs {
  const float* x_in; float* x_out; long sxb;
  const float* mag; long smb;
  const int* frames; const float* tab;
  int T_max;
};

// One radix-4 butterfly of pass NS of the forward transform (e^{-i ...}) in registers: v[1..3] times the pass's twiddles for
// q = j mod NS, then the 4-point DFT, in place.
template <int NS>
__device__ __forceinline__ void butterfly(float (&vr)[4], float (&vi)[4], const float* twc, const float* tws, int q) {
  if (NS > 1) {
#pragma unroll
    for (int r = 1; r < 4; ++r) {
      const float tc = twc[NS - 4 + (r - 1) * NS + q], ts = tws[NS - 4 + (r - 1) * NS + q];
      const float a = vr[r], bb = vi[r];
      vr[r] = a * tc - bb * ts;
      vi[r] = a * ts + bb * tc;
    }
  }
  const float t0r = vr[0] + vr[2], t0i = vi[0] + vi[2];
  const float t1r = vr[0] - vr[2], t1i = vi[0] - vi[2];
  const float t2r = vr[1] + vr[3], t2i = vi[1] + vi[3];
  const float t3r = vi[1] - vi[3], t3i = vr[3] - vr[1];      // -i (v1 - v3)
  vr[0] = t0r + t2r; vi[0] = t0i + t2i;
  vr[1] = t1r + t3r; vi[1] = t1i + t3i;
  vr[2] = t0r - t2r; vi[2] = t0i - t2i;
  vr[3] = t1r - t3r; vi[3] = t1i - t3i;
}

// Passes NS and 4 NS (NS = 1 or 16) with one trip through LDS.  Lane l does the pass-NS butterflies j = l + 64 c; output r of butterfly
// c lands on point P + r NS + 256 c with P = (l / NS) 4 NS + l mod NS < 256, and the pass-4NS butterfly j' = P + r NS reads exactly the
// points j' + 256 c: the lane's own 16 outputs are the inputs of its four butterflies of the next pass, so they stay in registers.
// ACT: the wave has a frame to transform (wave-uniform; the barriers are taken by all).
template <int NS>
__device__ __forceinline__ void fft_pass2(float* re, float* im, const float* twc, const float* tws, int lane, bool act) {
  float vr[4][4], vi[4][4];
  if (act) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = skew(lane + 64 * c + 256 * r);
        vr[c][r] = re[i];
        vi[c][r] = im[i];
      }
  }
  __syncthreads();
  if (act) {
#pragma unroll
    for (int c = 0; c < 4; ++c) butterfly<NS>(vr[c], vi[c], twc, tws, (lane + 64 * c) & (NS - 1));
    const int q0 = lane & (NS - 1), P = ((lane - q0) << 2) + q0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = P + r * NS, q = j & (4 * NS - 1);
      float ur[4], ui[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) { ur[c] = vr[c][r]; ui[c] = vi[c][r]; }
      butterfly<4 * NS>(ur, ui, twc, tws, q);
      const int base = ((j - q) << 2) + q;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        re[skew(base + o * 4 * NS)] = ur[o];
        im[skew(base + o * 4 * NS)] = ui[o];
      }
    }
  }
  __syncthreads();
}

// The last pass (NS = 256) alone: butterflies j = l + 64 c read j + 256 r and write the same points.
__device__ __forceinline__ void fft_pass_last(float* re, float* im, const float* twc, const float* tws, int lane, bool act) {
  constexpr int NS = NFFT / 4;
  float vr[4][4], vi[4][4];
  if (act) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = skew(lane + 64 * c + NS * r);
        vr[c][r] = re[i];
        vi[c][r] = im[i];
      }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      butterfly<NS>(vr[c], vi[c], twc, tws, lane + 64 * c);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = skew(lane + 64 * c + NS * r);
        re[i] = vr[c][r];
        im[i] = vi[c][r];
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void fft1024(float* re, float* im, const float* twc, const float* tws, int lane, bool act) {
  fft_pass2<1>(re, im, twc, tws, lane, act);
  fft_pass2<16>(re, im, twc, tws, lane, act);
  fft_pass_last(re, im, twc, tws, lane, act);
}

// M . (re, im) / |(re, im)|, (M, 0) at zero
__device__ __forceinline__ void project(float M, float re, float im, float& pr, float& pi) {
  const float s = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
  if (s == 0.f) { pr = M; pi = 0.f; return; }
  const float inv = M / __fsqrt_rn(s);
  pr = inv * re;
  pi = inv * im;
}

__global__ void __launch_bounds__(GL_THREADS, 4) gl_iter_kernel(GlArgs p) {
  extern __shared__ __attribute__((aligned(16))) float gl_smem[];
  float* twc = gl_smem;
  float* tws = gl_smem + NFFT;
  const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int T = min(max(p.frames[b], 0), p.T_max);
  const int NS = T > 0 ? T + 3 : 0;                  // blocks that carry signal
  const int sa = blockIdx.x * GL_OWN, sn = min(sa + GL_OWN, p.T_max + 4);
  float* xo = p.x_out + b * p.sxb;
  {                                                  // blocks of this tile at or past the row's signal: zeros
    float4* o4 = reinterpret_cast<float4*>(xo);
    for (int i = max(sa, NS) * (HOP / 4) + threadIdx.x; i < sn * (HOP / 4); i += GL_THREADS) o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (sa >= NS) return;
  const int se = min(sn, NS);
  for (int i = threadIdx.x; i < 2 * NFFT; i += GL_THREADS) gl_smem[i] = p.tab[NFFT + i];
  // ---- analysis input: z = hann . (x_a + i x_b) ----
  const int f0 = sa - 3, fa = f0 + 2 * w, fb = fa + 1;
  const bool va = fa >= 0 && fa < T, vb = fb >= 0 && fb < T, act = va || vb;
  float* re = gl_smem + 2 * NFFT + w * 2 * FSTR;
  float* im = re + FSTR;
  const float* xi = p.x_in + b * p.sxb;
  // Every global load of the wave is issued here, before the first transform: the 20 x 64 samples the two frames span (frame b is
  // frame a moved by one hop, so lane l needs samples l + 64 i, i < 20, once), the window, and the 2 x 9 magnitudes, which are not
  // needed before the projection and arrive behind the forward transform.
  float ma[NFFT / 128 + 1], mb[NFFT / 128 + 1];
  if (act) {
    float v[20], wn[16];
    const float* xf = xi + (long)fa * HOP + lane;      // formed for fa = -1 too (the left edge), but then read from i = 4 on only
#pragma unroll
    for (int i = 0; i < 20; ++i) v[i] = ((va && i < 16) || (vb && i >= 4)) ? xf[64 * i] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) wn[i] = p.tab[lane + 64 * i];
    const float* pa = p.mag + b * p.smb + (long)fa * NBINS;
    const float* pb = pa + NBINS;
#pragma unroll
    for (int m = 0; m <= NFFT / 128; ++m) {
      const int k = lane + 64 * m;
      ma[m] = va && k <= NFFT / 2 ? pa[k] : 0.f;
      mb[m] = vb && k <= NFFT / 2 ? pb[k] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int n = lane + 64 * i;
      re[skew(n)] = va ? wn[i] * v[i] : 0.f;
      im[skew(n)] = vb ? wn[i] * v[i + 4] : 0.f;
    }
  }
  __syncthreads();
  fft1024(re, im, twc, tws, lane, act);
  // ---- split the two spectra, project onto the magnitudes, rebuild the swapped input of the inverse transform ----
  if (act) {
#pragma unroll
    for (int m = 0; m <= NFFT / 128; ++m) {
      const int k = lane + 64 * m;
      if (k > NFFT / 2) break;
      const int k2 = (NFFT - k) & (NFFT - 1);
      const int i1 = skew(k), i2 = skew(k2);
      const float zr = re[i1], zi = im[i1], z2r = re[i2], z2i = im[i2];
      float par, pai, pbr, pbi;
      project(ma[m], zr + z2r, zi - z2i, par, pai);
      project(mb[m], zi + z2i, z2r - zr, pbr, pbi);
      // Y[k] = (par - pbi) + i (pai + pbr), Y[-k] = (par + pbi) + i (pbr - pai); stored with re and im exchanged.  k = 0 and 512
      // pair with themselves: pai and pbi are (signed) zeros there, so both stores write the same purely real pair.
      re[i2] = pbr - pai; im[i2] = par + pbi;
      re[i1] = pai + pbr; im[i1] = par - pbi;
    }
  }
  __syncthreads();
  fft1024(re, im, twc, tws, lane, act);
  // ---- overlap-add in frame order: frame a of a wave is in its im array, frame b in its re array ----
  const float4* win4 = reinterpret_cast<const float4*>(p.tab);
  for (int i = threadIdx.x; i < (se - sa) * (HOP / 4); i += GL_THREADS) {
    const int sl = i >> 6, j4 = (i & 63) * 4;
    float4 wn[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) wn[d] = win4[(d * HOP + j4) >> 2];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 3; d >= 0; --d) {
      const int m = sl + 3 - d, f = f0 + m;
      if (f < 0 || f >= T) continue;
      const float* y = gl_smem + 2 * NFFT + (m >> 1) * 2 * FSTR + ((m & 1) ? 0 : FSTR);
      const int o = skew(d * HOP + j4);                // a multiple of 4: the four samples share one skew
      acc[0] = __builtin_fmaf(wn[d].x, y[o], acc[0]);
      acc[1] = __builtin_fmaf(wn[d].y, y[o + 1], acc[1]);
      acc[2] = __builtin_fmaf(wn[d].z, y[o + 2], acc[2]);
      acc[3] = __builtin_fmaf(wn[d].w, y[o + 3], acc[3]);
    }
    const float sc = 1.f / (2 * NFFT);
    reinterpret_cast<float4*>(xo)[((sa + sl) * HOP + j4) >> 2] = make_float4(acc[0] * sc, acc[1] * sc, acc[2] * sc, acc[3] * sc);
  }
}

// ---- per-row x / max|x| ----
constexpr int PK_THREADS = 1024;
__global__ void __launch_bounds__(PK_THREADS) gl_peak_kernel(const float* x, float* y, long sxb, long S) {
  __shared__ float part[PK_THREADS / 64];
  const float* xi = x + blockIdx.x * sxb;
  float* yo = y + blockIdx.x * sxb;
  float m = 0.f;
  for (long i = threadIdx.x; i < S; i += PK_THREADS) m = fmaxf(m, fabsf(xi[i]));
  m = dx_wave_max(m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  float peak = 0.f;
#pragma unroll
  for (int i = 0; i < PK_THREADS / 64; ++i) peak = fmaxf(peak, part[i]);
  for (long i = threadIdx.x; i < S; i += PK_THREADS) {
    const float v = xi[i];
    yo[i] = peak > 0.f ? v / peak : v;
  }
}

// ---- NNLS mel -> linear -------------------------------------------------------------------------------------------------------------
// pack (int32 / f32 words): [0, 576) bin -> i0 | i1 << 16; [576, 1152) w0; [1152, 1728) w1; then per channel (128 each) the first
// bin, the count and the offset of its weights; then NN_CHW channel-major weights.  pinvT: [n_mels][576] fp32, zero past bin 512.
constexpr int NN_WAVES = 4, NN_THREADS = 64 * NN_WAVES;
constexpr int KP = 576, NPB = KP / 64;                 // padded bins, bins per lane
constexpr int NN_MAXCH = 128, NN_CHW = 1536;
constexpr int NN_PACK_WORDS = 3 * KP + 3 * NN_MAXCH + NN_CHW;

struct NnlsArgs {
  const float* mel; long smb; const int* lengths;
  const float* pinvT; const int* pack;
  float* X; long sxb;
  int T, n_mels, iters;
  float step;
};

__global__ void __launch_bounds__(NN_THREADS) nnls_mel_kernel(NnlsArgs p) {
  __shared__ int ch_lo[NN_MAXCH], ch_cnt[NN_MAXCH], ch_off[NN_MAXCH];
  __shared__ float chw[NN_CHW];
  __shared__ float sy[NN_WAVES][KP], sr[NN_WAVES][NN_MAXCH], sm[NN_WAVES][NN_MAXCH];
  const int b = blockIdx.y, t0 = blockIdx.x * NN_WAVES, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int len = min(max(p.lengths[b], 0), p.T), t = t0 + w, n_mels = p.n_mels;
  float* Xb = p.X + b * p.sxb;
  if (t0 >= len) {                                   // no valid frame in this tile: zeros only
    for (int i = threadIdx.x; i < NN_WAVES * NBINS; i += NN_THREADS)
      if (t0 + i / NBINS < p.T) Xb[(long)t0 * NBINS + i] = 0.f;
    return;
  }
  for (int i = threadIdx.x; i < NN_MAXCH; i += NN_THREADS) {      // clamped: a malformed pack cannot index outside LDS
    const int lo = min(max(p.pack[3 * KP + i], 0), NBINS - 1);
    const int cnt = i < n_mels ? min(max(p.pack[3 * KP + NN_MAXCH + i], 0), NBINS - lo) : 0;
    ch_lo[i] = lo; ch_cnt[i] = cnt;
    ch_off[i] = min(max(p.pack[3 * KP + 2 * NN_MAXCH + i], 0), NN_CHW - cnt);
  }
  for (int i = threadIdx.x; i < NN_CHW; i += NN_THREADS) chw[i] = __builtin_bit_cast(float, p.pack[3 * KP + 3 * NN_MAXCH + i]);
  const bool valid = t < len;
  for (int n = lane; n < NN_MAXCH; n += 64) sm[w][n] = valid && n < n_mels ? p.mel[b * p.smb + (long)n * p.T + t] : 0.f;
  int i0[NPB], i1[NPB];
  float w0[NPB], w1[NPB], x[NPB], y[NPB];
#pragma unroll
  for (int i = 0; i < NPB; ++i) {
    const int k = lane + 64 * i, id = p.pack[k];
    i0[i] = min(id & 0xFFFF, n_mels - 1);
    i1[i] = min((id >> 16) & 0xFFFF, n_mels - 1);
    w0[i] = __builtin_bit_cast(float, p.pack[KP + k]);
    w1[i] = __builtin_bit_cast(float, p.pack[2 * KP + k]);
    x[i] = 0.f;
  }
  __syncthreads();
  // ---- x0 = max(pinv(A) m, 0), channels in order ----
  for (int n = 0; n < n_mels; ++n) {
    const float mn = sm[w][n];
#pragma unroll
    for (int i = 0; i < NPB; ++i) x[i] = __builtin_fmaf(p.pinvT[(long)n * KP + lane + 64 * i], mn, x[i]);
  }
#pragma unroll
  for (int i = 0; i < NPB; ++i) y[i] = x[i] = fmaxf(x[i], 0.f);
  // ---- FISTA ----
  float tk = 1.f;
  for (int it = 0; it < p.iters; ++it) {
#pragma unroll
    for (int i = 0; i < NPB; ++i) sy[w][lane + 64 * i] = y[i];
    __syncthreads();
    for (int c = lane; c < n_mels; c += 64) {         // r = A y - m, each channel over its own run of bins, in bin order
      const int lo = ch_lo[c], cnt = ch_cnt[c], off = ch_off[c];
      float r = -sm[w][c];
      for (int i = 0; i < cnt; ++i) r = __builtin_fmaf(chw[off + i], sy[w][lo + i], r);
      sr[w][c] = r;
    }
    __syncthreads();
    const float tn = 0.5f * (1.f + __fsqrt_rn(1.f + 4.f * tk * tk)), beta = (tk - 1.f) / tn;
    tk = tn;
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
      const float g = __builtin_fmaf(w0[i], sr[w][i0[i]], w1[i] * sr[w][i1[i]]);
      const float xn = fmaxf(__builtin_fmaf(-p.step, g, y[i]), 0.f);
      y[i] = __builtin_fmaf(beta, xn - x[i], xn);
      x[i] = xn;
    }
  }
  if (t < p.T) {
#pragma unroll
    for (int i = 0; i < NPB; ++i) {
      const int k = lane + 64 * i;
      if (k < NBINS) Xb[(long)t * NBINS + k] = valid ? x[i] : 0.f;
    }
  }
}

}  // namespace

extern "C" {

int dx_gl_iter(const float* x_in, float* x_out, long sxb, const float* mag, long smb, const int* frames, const float* tab, int B,
               int T_max, int n_fft, int hop, void* stream) {
  DX_REQUIRE(x_in && x_out && mag && frames && tab, "dx_gl_iter: null pointer");
  DX_REQUIRE(n_fft == NFFT && hop == HOP, "dx_gl_iter: only n_fft = 1024, hop = 256 is implemented (got %d, %d)", n_fft, hop);
  DX_REQUIRE(x_in != x_out, "dx_gl_iter: x_out must not alias x_in (ping-pong two buffers)");
  DX_REQUIRE(B > 0 && B <= 65535 && T_max > 0 && T_max <= (1 << 22), "dx_gl_iter: bad shape (0 < B <= 65535, 0 < T_max <= 2^22)");
  DX_REQUIRE(sxb >= (long)HOP * T_max + NFFT && sxb % 4 == 0 && smb >= (long)T_max * NBINS,
             "dx_gl_iter: bad strides (sxb >= 256 T_max + 1024 and a multiple of 4, smb >= 513 T_max)");
  DX_REQUIRE(dx_aligned16(x_in) && dx_aligned16(x_out) && dx_aligned16(tab), "dx_gl_iter: x_in, x_out and tab must be 16-byte aligned");
  static bool configured = false;
  if (!configured) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(&gl_iter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)(GL_LDS_FLOATS * sizeof(float)));
    configured = true;
  }
  GlArgs a;
  a.x_in = x_in; a.x_out = x_out; a.sxb = sxb; a.mag = mag; a.smb = smb; a.frames = frames; a.tab = tab; a.T_max = T_max;
  hipLaunchKernelGGL(gl_iter_kernel, dim3(dx_cdiv(T_max + 4, GL_OWN), B), dim3(GL_THREADS), GL_LDS_FLOATS * sizeof(float),
                     (hipStream_t)stream, a);
  DX_LAUNCH_CHECK("dx_gl_iter");
  return DX_OK;
}

int dx_gl_peak_normalize(const float* x, float* y, long sxb, int B, long S, void* stream) {
  DX_REQUIRE(x && y, "dx_gl_peak_normalize: null pointer");
  DX_REQUIRE(B > 0 && B <= 65535 && S > 0 && sxb >= S, "dx_gl_peak_normalize: bad shape (0 < B <= 65535, 0 < S <= sxb)");
  hipLaunchKernelGGL(gl_peak_kernel, dim3(B), dim3(PK_THREADS), 0, (hipStream_t)stream, x, y, sxb, S);
  DX_LAUNCH_CHECK("dx_gl_peak_normalize");
  return DX_OK;
}

int dx_gl_layout(int* tile_blocks, int* pack_words) {
  DX_REQUIRE(tile_blocks && pack_words, "dx_gl_layout: null output");
  *tile_blocks = GL_OWN;
  *pack_words = NN_PACK_WORDS;
  return DX_OK;
}

int dx_nnls_mel(const float* mel, long smb, const int* lengths, const float* pinvT, const void* pack, float step, int iters, float* X,
                long sxb, int B, int T, int n_mels, int n_freq, void* stream) {
  DX_REQUIRE(mel && lengths && pinvT && pack && X, "dx_nnls_mel: null pointer");
  DX_REQUIRE(n_freq == NBINS && n_mels > 0 && n_mels <= NN_MAXCH, "dx_nnls_mel: only n_freq = 513 and 0 < n_mels <= 128 are implemented");
  DX_REQUIRE(B > 0 && B <= 65535 && T > 0 && iters >= 0 && step > 0.f, "dx_nnls_mel: bad shape (0 < B <= 65535, T > 0, iters >= 0, step > 0)");
  DX_REQUIRE(smb >= (long)n_mels * T && sxb >= (long)T * NBINS, "dx_nnls_mel: bad strides (smb >= n_mels T, sxb >= 513 T)");
  NnlsArgs a;
  a.mel = mel; a.smb = smb; a.lengths = lengths; a.pinvT = pinvT; a.pack = reinterpret_cast<const int*>(pack);
  a.X = X; a.sxb = sxb; a.T = T; a.n_mels = n_mels; a.iters = iters; a.step = step;
  hipLaunchKernelGGL(nnls_mel_kernel, dim3(dx_cdiv(T, NN_WAVES), B), dim3(NN_THREADS), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK("dx_nnls_mel");
  return DX_OK;
}

}  // extern "C"
