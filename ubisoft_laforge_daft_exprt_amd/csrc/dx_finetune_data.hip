// HiFi-GAN fine-tuning batches from a device-resident corpus (reference vocoder/dataset.py:118-148, the per-item work of
// HiFiGANFinetuneDataset.__getitem__ without the loss mel): one launch crops B (predicted mel, int16 audio) pairs into x (B, n_mels, fps)
// and y (B, segment) fp32.  The corpus is one int16 buffer (every utterance starts on a 16-byte boundary and the buffer ends on one) and
// one fp32 buffer of (n_mels, T_u) mels, with per-utterance offset and length tables.
#include <algorithm>

#include "dx_common.h"

namespace {

typedef short short8 __attribute__((ext_vector_type(8)));

constexpr int FT_THREADS = 256;

struct FtArgs {
  const short* wav; const long* wav_off; const int* wav_len;
  const float* mel; const long* mel_off; const int* mel_len;
  const int* utts; const int* order; const int* starts_in;
  uint64_t seed, counter;
  float* x; float* y; int* starts_out; int* utts_out;
  int n_utt, by_utt, segment, hop, fps, n_mels;
};

// Row b = blockIdx.x; the row's work items -- segment / 8 groups of 8 samples, then n_mels * fps mel cells -- are strided over the
// gridDim.y workgroups of the row.  A sample or a frame at or past the utterance's own length is written as 0 and never read (the last
// group of 8 may reach into the padding that follows every utterance), so a short utterance needs no path of its own: it starts at 0
// and the zeros are F.pad's.  An utterance index outside the tables gives a row of zeros.
__global__ __launch_bounds__(FT_THREADS) void ft_batch_kernel(FtArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int utt = a.utts ? a.utts[b] : a.order[b];
  const bool known = utt >= 0 && utt < a.n_utt;
  const long n_samples = known ? (long)a.wav_len[utt] : 0;
  const int T = known ? a.mel_len[utt] : 0;
  int start = 0;
  if (a.starts_in) {
    start = max(a.starts_in[b], 0);
  } else if (n_samples >= a.segment && T > a.fps) {
    // the reference's random.randint(0, T - fps - 1): the high word of the draw scaled to [0, T - fps)
    const uint64_t r = dx_rand64(a.seed, a.counter | (uint64_t)(a.by_utt ? utt : b));
    start = (int)(((r >> 32) * (uint64_t)(T - a.fps)) >> 32);
  }
  if (blockIdx.y == 0 && tid == 0) {
    if (a.starts_out) a.starts_out[b] = start;
    if (a.utts_out) a.utts_out[b] = utt;
  }
  const short* wav = a.wav + (known ? a.wav_off[utt] : 0);
  const float* mel = a.mel + (known ? a.mel_off[utt] : 0);
  const long first = (long)start * a.hop;                  // a multiple of hop: 16-byte aligned with the utterance's base when hop % 8 == 0
  float* y = a.y + (long)b * a.segment;
  float* x = a.x + (long)b * a.n_mels * a.fps;
  const int nvec = a.segment >> 3, ncell = a.n_mels * a.fps;
  for (int it = blockIdx.y * FT_THREADS + tid; it < nvec + ncell; it += gridDim.y * FT_THREADS) {
    if (it < nvec) {
      const long i = first + ((long)it << 3);
      f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
      if (i < n_samples) {
        const short8 s = *reinterpret_cast<const short8*>(wav + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lo[j] = i + j < n_samples ? (float)s[j] / 32768.0f : 0.f;
          hi[j] = i + j + 4 < n_samples ? (float)s[j + 4] / 32768.0f : 0.f;
        }
      }
      *reinterpret_cast<f32x4*>(y + ((long)it << 3)) = lo;
      *reinterpret_cast<f32x4*>(y + ((long)it << 3) + 4) = hi;
    } else {
      const int cell = it - nvec, c = cell / a.fps, f = cell - c * a.fps;
      const long t = (long)start + f;
      x[cell] = t < T ? mel[(long)c * T + t] : 0.f;
    }
  }
}

}  // namespace

extern "C" {

int dx_ft_batch(const short* wav, const long* wav_off, const int* wav_len, const float* mel, const long* mel_off, const int* mel_len,
                int n_utt, const int* utts, const int* order, long order_pos, long n_order, const int* starts_in, uint64_t seed,
                uint64_t counter, int by_utt, float* x, float* y, int* starts_out, int* utts_out, int B, int segment_size, int hop_size,
                int fps, int n_mels, void* stream) {
  DX_REQUIRE(wav && wav_off && wav_len && mel && mel_off && mel_len && x && y, "dx_ft_batch: null pointer");
  DX_REQUIRE(utts || order, "dx_ft_batch: null pointer (neither utts nor order)");
  DX_REQUIRE(B >= 1 && n_utt >= 1 && n_mels >= 1, "dx_ft_batch: bad sizes (B %d, n_utt %d, n_mels %d)", B, n_utt, n_mels);
  DX_REQUIRE(utts || (order_pos >= 0 && order_pos + B <= n_order), "dx_ft_batch: rows [%ld, %ld) are outside the order of %ld", order_pos,
             order_pos + B, n_order);
  DX_REQUIRE(hop_size >= 8 && hop_size % 8 == 0 && segment_size >= hop_size && segment_size % hop_size == 0 && fps >= 1 &&
             (long)fps * hop_size == segment_size, "dx_ft_batch: segment_size %d must be fps %d whole hops of %d samples (hop a multiple of 8)",
             segment_size, fps, hop_size);
  DX_REQUIRE((long)n_mels * fps < (1L << 30), "dx_ft_batch: n_mels %d x fps %d is too large", n_mels, fps);
  DX_REQUIRE(dx_aligned16(wav) && dx_aligned16(y), "dx_ft_batch: wav and y must be 16-byte aligned");
  FtArgs a{wav, wav_off, wav_len, mel, mel_off, mel_len, utts, utts ? nullptr : order + order_pos, starts_in, seed, counter,
           x, y, starts_out, utts_out, n_utt, by_utt ? 1 : 0, segment_size, hop_size, fps, n_mels};
  // one item per lane where the batch alone fills the chip; fewer, longer workgroups per row as B grows past that
  const int items = segment_size / 8 + n_mels * fps;
  const int chunks = std::max(1, std::min(dx_cdiv(items, FT_THREADS), dx_cdiv(1024, B)));
  hipLaunchKernelGGL(ft_batch_kernel, dim3(B, chunks), dim3(FT_THREADS), 0, (hipStream_t)stream, a);
  DX_LAUNCH_CHECK("dx_ft_batch");
  return DX_OK;
}

}  // extern "C"
