// Prosody-transfer row kernels: frames -> symbol means (extract_features.py:287-342), external-prosody conditioning
// (generate.py:165-185, :242-269 and model.py:975-1024, :1077-1087) and the fp32 -> 16-bit PCM rule (generate.py:327).
// Everything is fp32 or integer; no workspace, no atomics, every reduction in a fixed order that depends on the row alone, so a batch
// row is bitwise that utterance run alone.
#include "dx_common.h"

#include <algorithm>

// The conditioning arithmetic restates the reference's separate fp32 tensor operations: each one rounds on its own, and the value the
// reduction pass sums is the value the elementwise pass transforms.  No multiply-add fusion anywhere in this file.
#pragma clang fp contract(off)

namespace {

// fixed-order butterfly over the WIDTH lanes that share the high lane bits (WIDTH a power of two <= 64): every lane gets the sum
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = WIDTH / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- symbol prosody --------------------------------------------------------------------------------------------------------------
// One workgroup per utterance.  Symbols are taken 256 at a time: a block-wide exclusive scan of their durations gives each its first
// frame, then a group of 16 lanes averages one symbol (lane i sums frames off + i, off + i + 16, ... in order, then a 4-step butterfly).
constexpr int SP_THREADS = 256, SP_GROUP = 16;

__global__ __launch_bounds__(SP_THREADS) void symbol_prosody_kernel(const float* __restrict__ fe, const float* __restrict__ fp, long ldt,
                                                                    const long* __restrict__ dur_int, const int* __restrict__ in_lens,
                                                                    float* __restrict__ se, float* __restrict__ sp, int T, int L) {
  __shared__ int s_off[SP_THREADS], s_dur[SP_THREADS], s_wave[SP_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(max(in_lens[b], 0), L);
  const long* dur = dur_int + (long)b * L;
  const float* e = fe + (long)b * ldt;
  const float* p = fp + (long)b * ldt;
  float* oe = se + (long)b * L;
  float* op = sp + (long)b * L;
  int carry = 0;                                              // frames consumed by the symbols before this chunk (clamped to T)
  for (int l0 = 0; l0 < n; l0 += SP_THREADS) {
    const int l = l0 + tid;
    int d = 0;
    if (l < n) d = (int)min(max(dur[l], 0L), (long)T);
    int incl = d;                                             // inclusive scan inside the wave; sums stay below 64 T + T
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before = min(before + s_wave[w], T);
    const int first = min(before + (incl - d), T);            // frames past T are never read, whatever the durations say
    s_off[tid] = first;
    s_dur[tid] = d;
    int total = carry;
    for (int w = 0; w < SP_THREADS / 64; ++w) total = min(total + s_wave[w], T);
    carry = total;
    __syncthreads();
    const int g = tid / SP_GROUP, gl = tid % SP_GROUP;
    const int count = min(SP_THREADS, n - l0);
    for (int s = g; s < count; s += SP_THREADS / SP_GROUP) {
      const int d_s = s_dur[s], t0 = s_off[s], t1 = min(t0 + d_s, T);
      float esum = 0.f, psum = 0.f, voiced = 0.f;
      for (int t = t0 + gl; t < t1; t += SP_GROUP) {
        esum += e[t];
        const float v = p[t];
        if (v > 0.f) { psum += v; voiced += 1.f; }
      }
      esum = group_sum<SP_GROUP>(esum);
      psum = group_sum<SP_GROUP>(psum);
      voiced = group_sum<SP_GROUP>(voiced);
      if (gl == 0) {
        oe[l0 + s] = d_s > 0 ? esum / (float)d_s : 0.f;
        op[l0 + s] = voiced > 0.f ? psum / voiced : 0.f;
      }
    }
    __syncthreads();
  }
  for (int l = n + tid; l < L; l += SP_THREADS) { oe[l] = 0.f; op[l] = 0.f; }
}

// ---- conditioning ----------------------------------------------------------------------------------------------------------------
struct CondArgs {
  const float *energy, *pitch;
  const long* dur_int;
  const int* in_lens;
  const float *energy_factors, *pitch_factors, *stats, *source;
  float alpha_energy, alpha_pitch;
  int mode, normalize;
  float *energy_out, *pitch_out;
  int L;
};

// generate.py:165-185 + :265-269 for one value, each operation rounded on its own like the reference's separate tensor ops
__device__ __forceinline__ float normalise(float v, bool has_source, float src_mean, float src_std, float tgt_mean, float tgt_std, float alpha) {
  if (v == 0.f) return 0.f;
  if (has_source) v = (v - src_mean) / src_std * tgt_std + tgt_mean;
  v = (v - tgt_mean) / tgt_std;
  return v * alpha;
}

constexpr int PC_THREADS = 256;

// One workgroup per utterance: the voiced mean of the conditioned pitch in a fixed order (multiply only), then the elementwise pass.
__global__ __launch_bounds__(PC_THREADS) void prosody_condition_kernel(CondArgs a) {
  __shared__ float s_sum[PC_THREADS / 64], s_cnt[PC_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, L = a.L;
  const int n = min(max(a.in_lens[b], 0), L);
  const long row = (long)b * L;
  const bool has_source = a.source != nullptr;
  float e_mean = 0.f, e_std = 1.f, p_mean = 0.f, p_std = 1.f, se_mean = 0.f, se_std = 1.f, sp_mean = 0.f, sp_std = 1.f;
  if (a.stats) { e_mean = a.stats[4 * b]; e_std = a.stats[4 * b + 1]; p_mean = a.stats[4 * b + 2]; p_std = a.stats[4 * b + 3]; }
  if (has_source) { se_mean = a.source[0]; se_std = a.source[1]; sp_mean = a.source[2]; sp_std = a.source[3]; }

  // the pitch after steps 1-7, identical in both passes
  auto pitch_at = [&](int l) -> float {
    float v = a.pitch[row + l];
    if (a.normalize) v = normalise(v, has_source, sp_mean, sp_std, p_mean, p_std, a.alpha_pitch);
    if (a.dur_int && a.dur_int[row + l] == 0) v = 0.f;
    return v;
  };

  float voiced_mean = 0.f;
  if (a.mode == 2) {
    float sum = 0.f, cnt = 0.f;
    for (int l = tid; l < n; l += PC_THREADS) {
      const float v = pitch_at(l);
      if (v != 0.f) { sum += v; cnt += 1.f; }
    }
    sum = group_sum<64>(sum);
    cnt = group_sum<64>(cnt);
    if ((tid & 63) == 0) { s_sum[tid >> 6] = sum; s_cnt[tid >> 6] = cnt; }
    __syncthreads();
    sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    cnt = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    voiced_mean = cnt > 0.f ? sum / cnt : 0.f;               // an all-unvoiced row has no voiced value to move: the mean is never used
  }

  for (int l = tid; l < L; l += PC_THREADS) {
    float e = 0.f, p = 0.f;
    if (l < n) {
      e = a.energy[row + l];
      if (a.normalize) e = normalise(e, has_source, se_mean, se_std, e_mean, e_std, a.alpha_energy);
      if (a.energy_factors) e *= a.energy_factors[row + l];
      if (a.dur_int && a.dur_int[row + l] == 0) e = 0.f;
      p = pitch_at(l);
      if (p != 0.f) {
        const float f = a.pitch_factors ? a.pitch_factors[row + l] : 0.f;
        if (a.mode == 1) {                                   // model.py:975-994: shift in Hz, back to the normalised log domain
          // in double, rounded once: an fp32 log near 5 is uncertain by 5e-7, and 1 / std (about 4) multiplies that
          const double hz = exp((double)p_std * (double)p + (double)p_mean) + (double)f;
          p = (float)((log(hz) - (double)p_mean) / (double)p_std);
        } else if (a.mode == 2) {                            // model.py:996-1024: scale the deviation from the voiced mean
          p = p + (p - voiced_mean) * f;
        }
      }
    }
    a.energy_out[row + l] = e;
    a.pitch_out[row + l] = p;
  }
}

// ---- 16-bit PCM -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ short pcm_of(float x) {
  const float y = fminf(fmaxf(x * 32767.5f, -32768.f), 32767.f);
  return (short)(int)y;                                       // conversion truncates toward zero, as numpy's astype
}

typedef short short8 __attribute__((ext_vector_type(8)));

// Row b of S samples: the samples before the first index whose flat offset is a multiple of 8 and those after the last whole group of 8
// go one by one (first workgroup of the row), the groups between as two 16-byte loads and one 16-byte store; a group at or past the
// row's length is stored as zeros without being read.
__global__ __launch_bounds__(256) void pcm16_kernel(const float* __restrict__ audio, const int* __restrict__ lens, short* __restrict__ pcm, long S) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const long base = (long)b * S;
  const long n = min(max((long)lens[b], 0L), S);
  const long head = min((long)((8 - (base & 7)) & 7), S);
  const long nvec = (S - head) >> 3;
  const long tail0 = head + (nvec << 3);
  const float* in = audio + base;
  short* out = pcm + base;
  for (long v = (long)blockIdx.x * 256 + tid; v < nvec; v += (long)gridDim.x * 256) {
    const long i = head + (v << 3);
    short8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < n) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(in + i);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(in + i + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = i + j < n ? pcm_of(x0[j]) : (short)0;
        r[j + 4] = i + j + 4 < n ? pcm_of(x1[j]) : (short)0;
      }
    }
    *reinterpret_cast<short8*>(out + i) = r;
  }
  if (blockIdx.x == 0) {
    long i = -1;
    if (tid < head) i = tid;
    else if (tid >= 8 && tid - 8 < S - tail0) i = tail0 + (tid - 8);
    if (i >= 0) out[i] = i < n ? pcm_of(in[i]) : (short)0;
  }
}

}  // namespace

extern "C" {

int dx_symbol_prosody(const float* frames_energy, const float* frames_pitch, long ldt, const long* dur_int, const int* in_lens,
                      float* sym_energy, float* sym_pitch, int B, int T, int L, void* stream) {
  DX_REQUIRE(frames_energy && frames_pitch && dur_int && in_lens && sym_energy && sym_pitch, "dx_symbol_prosody: null pointer");
  DX_REQUIRE(B > 0 && L > 0 && T >= 0 && ldt >= T, "dx_symbol_prosody: bad sizes (B %d, T %d, L %d, ldt %ld)", B, T, L, ldt);
  DX_REQUIRE(T < (1 << 24), "dx_symbol_prosody: T %d: frame counts are summed in fp32 and must stay below 2^24", T);
  hipLaunchKernelGGL(symbol_prosody_kernel, dim3(B), dim3(SP_THREADS), 0, (hipStream_t)stream, frames_energy, frames_pitch, ldt, dur_int,
                     in_lens, sym_energy, sym_pitch, T, L);
  DX_LAUNCH_CHECK("dx_symbol_prosody");
  return DX_OK;
}

int dx_prosody_condition(const float* energy, const float* pitch, const long* dur_int, const int* in_lens, const float* energy_factors,
                         const float* pitch_factors, const float* stats, const float* source, int has_source, float alpha_energy,
                         float alpha_pitch, int mode, int normalize, float* energy_out, float* pitch_out, int B, int L, void* stream) {
  DX_REQUIRE(energy && pitch && in_lens && energy_out && pitch_out, "dx_prosody_condition: null pointer");
  DX_REQUIRE(B > 0 && L > 0, "dx_prosody_condition: bad sizes (B %d, L %d)", B, L);
  DX_REQUIRE(mode >= 0 && mode <= 2, "dx_prosody_condition: mode %d (0 none, 1 add, 2 multiply)", mode);
  DX_REQUIRE(mode == 0 || pitch_factors, "dx_prosody_condition: a pitch transform needs pitch_factors");
  DX_REQUIRE(stats || (!normalize && mode != 1), "dx_prosody_condition: normalisation and the add transform need the stats table");
  DX_REQUIRE(!has_source || (source && normalize), "dx_prosody_condition: has_source needs source and normalize");
  CondArgs a{energy, pitch, dur_int, in_lens, energy_factors, pitch_factors, stats, has_source ? source : nullptr,
             alpha_energy, alpha_pitch, mode, normalize, energy_out, pitch_out, L};
  hipLaunchKernelGGL(prosody_condition_kernel, dim3(B), dim3(PC_THREADS), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK("dx_prosody_condition");
  return DX_OK;
}

int dx_pcm16(const float* audio, const int* sample_lengths, short* pcm, int B, long S, void* stream) {
  DX_REQUIRE(audio && sample_lengths && pcm, "dx_pcm16: null pointer");
  DX_REQUIRE(B > 0 && B <= 65535 && S > 0, "dx_pcm16: bad sizes (B %d, S %ld)", B, S);
  DX_REQUIRE(((uintptr_t)audio & 15) == 0 && ((uintptr_t)pcm & 15) == 0, "dx_pcm16: audio and pcm must be 16-byte aligned");
  const long nvec = S / 8 + 1;
  const int blocks = (int)std::min<long>((nvec + 255) / 256, 4096);
  hipLaunchKernelGGL(pcm16_kernel, dim3(blocks, B), dim3(256), 0, (hipStream_t)stream, audio, sample_lengths, pcm, S);
  DX_LAUNCH_CHECK("dx_pcm16");
  return DX_OK;
}

}  // extern "C"
