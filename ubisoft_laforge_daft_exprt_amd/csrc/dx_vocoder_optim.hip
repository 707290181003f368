// The optimiser step of HiFi-GAN fine-tuning (reference vocoder/finetune_hifigan.py:130-135, :226, :243): for every weight-normed
// tensor the backward of the weight norm, torch's AdamW on g and v, and the fold of the stepped pair into the convolution weight, in
// ONE pass over the row; for every other tensor plain AdamW.  One launch steps all tensors of one optimiser.
//
// Per row r of a weight-normed tensor (v (R, n) rows contiguous, g (R), dW in v's layout):
//   nrm = |v_r|,  dg = <dW_r, v_r> / nrm,  dv = (g / nrm) (dW_r - (dg / nrm) v_r),  AdamW on (g, dg) and on (v_r, dv),
//   W_r = g' v'_r / |v'_r| from the values as stored.
// The row stays in registers between its three reductions: dW, v, g and the four moments are read once, v, g, the moments and W written
// once (32 bytes per element), in 16-byte accesses.  A row of at most 1024 elements is one wave's (four rows to a workgroup), a longer
// one (up to 6144) a workgroup's.  Rows with n % 4 != 0 take 4-byte accesses and read the row once per pass.  The three reductions and
// the weight norm's backward run in double (see wave_sum), AdamW itself in fp32 as torch's does.  Every sum is a fixed tree -- per-lane
// partial sums in slot order, the wave butterfly, the four waves' sums in a fixed order -- that depends on n alone: no atomics, and the bits do not depend on which
// other jobs share the launch.
//
// The job table lives in device memory and is laid out on the host by dx_wn_adamw_table: njobs entries (Job below), then one
// (job, first row or chunk) pair per workgroup.
#include "dx_common.h"
#include <math.h>

namespace {

enum { MODE_PLAIN = 0, MODE_WAVE_V = 1, MODE_WAVE_S = 2, MODE_BLOCK_V = 3, MODE_BLOCK_S = 4 };
constexpr int WAVE_MAX = 1024;       // the longest row one wave holds: 64 lanes x 16 elements
constexpr int ROW_MAX = 6144;        // the longest row at all: 256 threads x 24 elements (212 VGPRs: two waves per SIMD)
constexpr int PLAIN_CHUNK = 2048;    // elements of a plain tensor per workgroup: 256 threads x two 16-byte accesses
constexpr int JOB_WORDS = 11;        // the host descriptor: kind, R, n, v, g, dW, m_v, s_v, m_g, s_g, W

struct Job {                         // 80 bytes
  float* v; float* g; const float* dW; float* m_v; float* s_v; float* m_g; float* s_g; float* W;
  int mode, R, n, pad;
};

struct Hyper {                       // formed on the host in double, each rounded once
  float decay;                       // 1 - lr wd
  float step_size;                   // lr / (1 - b1^step)
  float b1, omb1, b2, omb2;          // the betas and 1 - beta
  float bc2_sqrt;                    // sqrt(1 - b2^step)
  float eps;
};

// torch.optim.AdamW on one element (amsgrad = False, maximize = False)
__device__ __forceinline__ void adamw_one(float& p, float grad, float& m, float& s, const Hyper& h) {
  p = p * h.decay;
  m = h.b1 * m + h.omb1 * grad;
  s = h.b2 * s + h.omb2 * (grad * grad);
  p = p - h.step_size * (m / (sqrtf(s) / h.bc2_sqrt + h.eps));
}

template <int VEC> __device__ __forceinline__ void load_slot(const float* p, float (&x)[VEC]) {
  if constexpr (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
  } else {
    x[0] = *p;
  }
}
template <int VEC> __device__ __forceinline__ void store_slot(float* p, const float (&x)[VEC]) {
  if constexpr (VEC == 4) {
    f32x4 t; t[0] = x[0]; t[1] = x[1]; t[2] = x[2]; t[3] = x[3];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    *p = x[0];
  }
}

// The row's reductions run in double.  With fresh moments AdamW's update is lr dv / (|dv| + eps), and where dW_r and (dg / nrm) v_r
// cancel to |dv| < eps the update is linear in dv with slope lr / eps: an fp32 dot product's 1e-6 relative error in dg then moves the
// parameter by more than its own rounding (seen on a 512 x 656 layer of the MSD).  The kernel is memory bound: two DFMAs per element
// are free.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum over the row's owner (a wave, or the four waves of the workgroup): every thread gets the same bits
template <int THREADS> __device__ __forceinline__ double row_sum(double x, double* part, int tid) {
  x = wave_sum(x);
  if constexpr (THREADS == 64) return x;
  if ((tid & 63) == 0) part[tid >> 6] = x;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// |x_r|^2 of the row held in slots: the ONE definition of the norm that the step and dx_wn_fold share
template <int THREADS, int CAP, int VEC> __device__ __forceinline__ double row_sumsq(const float (&x)[CAP][VEC], double* part, int tid) {
  double ss = 0.0;
#pragma unroll
  for (int j = 0; j < CAP; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) ss = fma((double)x[j][e], (double)x[j][e], ss);
  return row_sum<THREADS>(ss, part, tid);
}

// W_r = g v_r / |v_r| (torch._weight_norm: v * (g / norm)); slots past the row hold zeros and are not stored
template <int THREADS, int CAP, int VEC>
__device__ __forceinline__ void fold_row(const float (&v)[CAP][VEC], float g, float* W, int nv, double* part, int tid) {
  const float scale = (float)((double)g / sqrt(row_sumsq<THREADS, CAP, VEC>(v, part, tid)));
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    const int idx = j * THREADS + tid;
    if (idx < nv) {
      float w[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) w[e] = v[j][e] * scale;
      store_slot<VEC>(W + (long)idx * VEC, w);
    }
  }
}

// One row of n % 4 == 0 elements, held in registers.  tid: the thread's index among the row's THREADS owners; part: 12 doubles of LDS
// (touched only when THREADS == 256).
template <int THREADS, int CAP, bool STEP>
__device__ __forceinline__ void wn_row(const Job& J, int row, int tid, double* part, const Hyper& h) {
  constexpr int VEC = 4;
  const int nv = J.n / VEC;
  const long off = (long)row * J.n;
  float v[CAP][VEC];
  if constexpr (!STEP) {
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      const int idx = j * THREADS + tid;
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[j][e] = 0.f;
      if (idx < nv) load_slot<VEC>(J.v + off + (long)idx * VEC, v[j]);
    }
    fold_row<THREADS, CAP, VEC>(v, J.g[row], J.W + off, nv, part, tid);
  } else {
    float d[CAP][VEC], m[CAP][VEC], s[CAP][VEC];
    float g = J.g[row], mg = J.m_g[row], sg = J.s_g[row];      // every thread reads them (one address), thread 0 writes them at the end
#pragma unroll
    for (int j = 0; j < CAP; ++j) {                          // everything the row reads, issued before the first reduction
      const int idx = j * THREADS + tid;
#pragma unroll
      for (int e = 0; e < VEC; ++e) v[j][e] = d[j][e] = m[j][e] = s[j][e] = 0.f;
      if (idx < nv) {
        const long at = off + (long)idx * VEC;
        load_slot<VEC>(J.v + at, v[j]);
        load_slot<VEC>(J.dW + at, d[j]);
        load_slot<VEC>(J.m_v + at, m[j]);
        load_slot<VEC>(J.s_v + at, s[j]);
      }
    }
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) dot = fma((double)d[j][e], (double)v[j][e], dot);
    const double nrm = sqrt(row_sumsq<THREADS, CAP, VEC>(v, part, tid));
    dot = row_sum<THREADS>(dot, part + 4, tid);
    const double dg = dot / nrm;
    const double c1 = (double)g / nrm, c2 = dg / nrm;
    adamw_one(g, (float)dg, mg, sg, h);
#pragma unroll
    for (int j = 0; j < CAP; ++j) {
      const int idx = j * THREADS + tid;
      if (idx < nv) {
        const long at = off + (long)idx * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float dv = (float)(c1 * ((double)d[j][e] - c2 * (double)v[j][e]));
          adamw_one(v[j][e], dv, m[j][e], s[j][e], h);
        }
        store_slot<VEC>(J.v + at, v[j]);
        store_slot<VEC>(J.m_v + at, m[j]);
        store_slot<VEC>(J.s_v + at, s[j]);
      }
    }
    if (tid == 0) { J.g[row] = g; J.m_g[row] = mg; J.s_g[row] = sg; }
    fold_row<THREADS, CAP, VEC>(v, g, J.W + off, nv, part + 8, tid);      // from the values as stored
  }
}

// |v_r|^2 and W_r of a row read from memory: the 4-byte paths' definition of the norm, shared by their step and their fold
template <int THREADS> __device__ __forceinline__ void fold_row_mem(const float* v, float g, float* W, int n, double* part, int tid) {
  double ss = 0.0;
  for (int i = tid; i < n; i += THREADS) ss = fma((double)v[i], (double)v[i], ss);
  const float scale = (float)((double)g / sqrt(row_sum<THREADS>(ss, part, tid)));
  for (int i = tid; i < n; i += THREADS) W[i] = v[i] * scale;
}

// One row whose length is no multiple of 4 (in the three models: the first layers' rows of 5 and 15 taps): 4-byte accesses, the row
// read again by each pass -- from the cache; every thread reads back only what it wrote itself.
template <int THREADS, bool STEP>
__device__ __forceinline__ void wn_row_odd(const Job& J, int row, int tid, double* part, const Hyper& h) {
  const int n = J.n;
  const long off = (long)row * n;
  float* v = J.v + off;
  float g = J.g[row];
  if constexpr (STEP) {
    const float* d = J.dW + off;
    float mg = J.m_g[row], sg = J.s_g[row];
    double ss = 0.0, dot = 0.0;
    for (int i = tid; i < n; i += THREADS) { ss = fma((double)v[i], (double)v[i], ss); dot = fma((double)d[i], (double)v[i], dot); }
    const double nrm = sqrt(row_sum<THREADS>(ss, part + 4, tid));
    dot = row_sum<THREADS>(dot, part + 8, tid);
    const double dg = dot / nrm;
    const double c1 = (double)g / nrm, c2 = dg / nrm;
    adamw_one(g, (float)dg, mg, sg, h);
    for (int i = tid; i < n; i += THREADS) {
      float p = v[i], m = J.m_v[off + i], s = J.s_v[off + i];
      adamw_one(p, (float)(c1 * ((double)d[i] - c2 * (double)p)), m, s, h);
      v[i] = p; J.m_v[off + i] = m; J.s_v[off + i] = s;
    }
    if (tid == 0) { J.g[row] = g; J.m_g[row] = mg; J.s_g[row] = sg; }
  }
  fold_row_mem<THREADS>(v, g, J.W + off, n, part, tid);
}

// plain AdamW on one chunk of PLAIN_CHUNK elements; the last chunk also takes the n % 4 tail
__device__ __forceinline__ void plain_chunk(const Job& J, int chunk, int tid, const Hyper& h) {
  const int n4 = J.n / 4;
#pragma unroll
  for (int j = 0; j < PLAIN_CHUNK / 1024; ++j) {
    const long i = (long)chunk * (PLAIN_CHUNK / 4) + j * 256 + tid;
    if (i < n4) {
      float p[4], d[4], m[4], s[4];
      load_slot<4>(J.v + 4 * i, p); load_slot<4>(J.dW + 4 * i, d); load_slot<4>(J.m_v + 4 * i, m); load_slot<4>(J.s_v + 4 * i, s);
#pragma unroll
      for (int e = 0; e < 4; ++e) adamw_one(p[e], d[e], m[e], s[e], h);
      store_slot<4>(J.v + 4 * i, p); store_slot<4>(J.m_v + 4 * i, m); store_slot<4>(J.s_v + 4 * i, s);
    }
  }
  const int i = 4 * n4 + tid;
  if (chunk == (J.n - 1) / PLAIN_CHUNK && tid < 4 && i < J.n) adamw_one(J.v[i], J.dW[i], J.m_v[i], J.s_v[i], h);
}

template <bool STEP>
__global__ __launch_bounds__(256) void wn_kernel(const Job* __restrict__ jobs, const int2* __restrict__ index, const Hyper h) {
  __shared__ double part[12];
  const int2 where = index[blockIdx.x];
  const Job J = jobs[where.x];
  const int tid = threadIdx.x;
  if (J.mode == MODE_PLAIN) {
    if constexpr (STEP) plain_chunk(J, where.y, tid, h);
  } else if (J.mode == MODE_WAVE_V || J.mode == MODE_WAVE_S) {
    const int row = where.y + (tid >> 6);                   // four rows to a workgroup; no barrier on this path
    if (row < J.R) {
      if (J.mode == MODE_WAVE_V) wn_row<64, WAVE_MAX / 256, STEP>(J, row, tid & 63, part, h);
      else wn_row_odd<64, STEP>(J, row, tid & 63, part, h);
    }
  } else if (J.mode == MODE_BLOCK_V) {
    wn_row<256, ROW_MAX / 1024, STEP>(J, where.y, tid, part, h);
  } else {
    wn_row_odd<256, STEP>(J, where.y, tid, part, h);
  }
}

int job_mode(long kind, long n) {
  if (kind == 0) return MODE_PLAIN;
  if (n <= WAVE_MAX) return n % 4 == 0 ? MODE_WAVE_V : MODE_WAVE_S;
  return n % 4 == 0 ? MODE_BLOCK_V : MODE_BLOCK_S;
}

long job_blocks(int mode, long R, long n) {
  if (mode == MODE_PLAIN) return (n + PLAIN_CHUNK - 1) / PLAIN_CHUNK;
  if (mode == MODE_WAVE_V || mode == MODE_WAVE_S) return (R + 3) / 4;
  return R;
}

bool aligned(long p, int a) { return ((uintptr_t)p % a) == 0; }

// every descriptor checked -> the number of workgroups, or -1 with the error set
long check_jobs(const char* who, const long* jobs, int njobs) {
  if (!jobs || njobs < 1) { dx_set_error("%s: no jobs", who); return -1; }
  long blocks = 0;
  for (int j = 0; j < njobs; ++j) {
    const long* d = jobs + (long)j * JOB_WORDS;
    const long kind = d[0], R = d[1], n = d[2];
    if (kind != 0 && kind != 1) { dx_set_error("%s: job %d: kind must be 0 (plain) or 1 (weight-normed), got %ld", who, j, kind); return -1; }
    if (R < 1 || n < 1 || R > 0x7fffffffL || n > 0x7fffffffL || (kind == 0 && R != 1)) {
      dx_set_error("%s: job %d: bad shape R = %ld, n = %ld (a plain job has R = 1)", who, j, R, n); return -1;
    }
    if (kind == 1 && n > ROW_MAX) { dx_set_error("%s: job %d: a row of %ld elements; the kernel holds rows of at most %d", who, j, n, ROW_MAX); return -1; }
    const long v = d[3], g = d[4], dW = d[5], m_v = d[6], s_v = d[7], m_g = d[8], s_g = d[9], W = d[10];
    if (!v || !dW || !m_v || !s_v || (kind == 1 && (!g || !m_g || !s_g || !W))) { dx_set_error("%s: job %d: null pointer", who, j); return -1; }
    if (!aligned(m_v, 16) || !aligned(s_v, 16) || !aligned(m_g, 4) || !aligned(s_g, 4)) {
      dx_set_error("%s: job %d: the moments must be 16-byte aligned (those of g: 4)", who, j); return -1;
    }
    if (!aligned(v, 16) || !aligned(dW, 16) || !aligned(W, 16) || !aligned(g, 4)) {
      dx_set_error("%s: job %d: v, dW and W must be 16-byte aligned (g: 4)", who, j); return -1;
    }
    blocks += job_blocks(job_mode(kind, n), R, n);
    if (blocks > 0x7fffffffL) { dx_set_error("%s: more than 2^31 workgroups", who); return -1; }
  }
  return blocks;
}

long table_bytes(int njobs, long blocks) { return (long)njobs * sizeof(Job) + blocks * sizeof(int2); }

int launch_args_ok(const char* who, const void* table, int njobs, int blocks) {
  DX_REQUIRE(table, "%s: null table", who);
  DX_REQUIRE(aligned((long)(uintptr_t)table, 16), "%s: the table must be 16-byte aligned", who);
  DX_REQUIRE(njobs >= 1 && blocks >= 1, "%s: njobs and blocks must be positive, got %d and %d", who, njobs, blocks);
  return DX_OK;
}

}  // namespace

extern "C" {

int dx_wn_adamw_table_size(const long* jobs, int njobs, long* bytes, int* blocks) {
  DX_REQUIRE(bytes && blocks, "dx_wn_adamw_table_size: null output pointer");
  const long nb = check_jobs("dx_wn_adamw_table_size", jobs, njobs);
  if (nb < 0) return DX_ERR_ARG;
  *bytes = table_bytes(njobs, nb);
  *blocks = (int)nb;
  return DX_OK;
}

int dx_wn_adamw_table(const long* jobs, int njobs, void* table, long bytes) {
  const long nb = check_jobs("dx_wn_adamw_table", jobs, njobs);
  if (nb < 0) return DX_ERR_ARG;
  DX_REQUIRE(table, "dx_wn_adamw_table: null table");
  DX_REQUIRE(bytes == table_bytes(njobs, nb), "dx_wn_adamw_table: the table is %ld bytes, dx_wn_adamw_table_size reports %ld", bytes,
             table_bytes(njobs, nb));
  Job* J = reinterpret_cast<Job*>(table);
  int2* index = reinterpret_cast<int2*>(J + njobs);
  long b = 0;
  for (int j = 0; j < njobs; ++j) {
    const long* d = jobs + (long)j * JOB_WORDS;
    const int mode = job_mode(d[0], d[2]);
    J[j] = Job{(float*)d[3], (float*)d[4], (const float*)d[5], (float*)d[6], (float*)d[7], (float*)d[8], (float*)d[9], (float*)d[10],
               mode, (int)d[1], (int)d[2], 0};
    const long nbj = job_blocks(mode, d[1], d[2]);
    const int per = (mode == MODE_WAVE_V || mode == MODE_WAVE_S) ? 4 : 1;
    for (long i = 0; i < nbj; ++i) index[b++] = make_int2(j, (int)(i * per));
  }
  return DX_OK;
}

int dx_wn_adamw(const void* table, int njobs, int blocks, double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                void* stream) {
  if (int rc = launch_args_ok("dx_wn_adamw", table, njobs, blocks)) return rc;
  DX_REQUIRE(step >= 1, "dx_wn_adamw: step must be at least 1, got %d", step);
  DX_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "dx_wn_adamw: betas must lie in [0, 1)");
  DX_REQUIRE(lr >= 0.0 && eps >= 0.0 && weight_decay >= 0.0 && lr < INFINITY && eps < INFINITY && weight_decay < INFINITY,
             "dx_wn_adamw: lr, eps and weight_decay must be finite and not negative");
  const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
  const Hyper h{(float)(1.0 - lr * weight_decay), (float)(lr / bc1), (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                (float)sqrt(bc2), (float)eps};
  const Job* J = reinterpret_cast<const Job*>(table);
  hipLaunchKernelGGL(wn_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, J, reinterpret_cast<const int2*>(J + njobs), h);
  DX_LAUNCH_CHECK("dx_wn_adamw");
  return DX_OK;
}

int dx_wn_fold(const void* table, int njobs, int blocks, void* stream) {
  if (int rc = launch_args_ok("dx_wn_fold", table, njobs, blocks)) return rc;
  const Job* J = reinterpret_cast<const Job*>(table);
  hipLaunchKernelGGL(wn_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, J, reinterpret_cast<const int2*>(J + njobs), Hyper{});
  DX_LAUNCH_CHECK("dx_wn_fold");
  return DX_OK;
}

}  // extern "C"
