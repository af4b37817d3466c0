// Exponential moving average of the weights for gfx950 (HBM-bound streaming: two streams in, one out).
//
// Replaces the per-parameter tensor arithmetic of diffusers 0.20.0 `training_utils.EMAModel.step`
//     s_param.sub_(one_minus_decay * (s_param - param))        (requires_grad)
//     s_param.copy_(param)                                     (frozen)
// -- 282 x 3 small launches per training step on the default network -- by ONE table-driven launch.  Every operation is
// rounded to fp32 on its own (fma contraction disabled for this file), so the shadows are bit-identical to torch-CPU.
//
// There is one kernel and no second "flat" one: the Python wrapper merges neighbouring jobs that are contiguous in both
// buffers, and once AdamW has moved the parameters into its slab the table is a single job.
#include "dsg_common.h"

// HIP's __fmul_rn/__fsub_rn are plain operators (contractible); forbid fma contraction for this TU instead.
#pragma clang fp contract(off)

namespace dsg {

constexpr int kEmaChunk = DSG_EMA_CHUNK;
constexpr int kEmaRows = kEmaChunk / (256 * 4);  // float4 rows of the workgroup per chunk
static_assert(kEmaChunk % (256 * 4) == 0, "a chunk is a whole number of 256-lane float4 rows: chunk starts keep a job's 16-byte alignment");

// the table hands the kernel generic pointers; they are device memory: global_load / global_store instead of the flat forms
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;

__device__ __forceinline__ float ema_elem(float s, float p, float omd) { return __fsub_rn(s, __fmul_rn(omd, __fsub_rn(s, p))); }
__device__ __forceinline__ f32x4 ema_elem4(f32x4 s, f32x4 p, float omd) {
  const f32x4 t = s - p;
  const f32x4 u = t * omd;
  return s - u;
}

// Chunk c of the launch belongs to the job j with first[j] <= c < first[j + 1] (bisection; the same for every lane of the
// workgroup) and covers elements [k * kEmaChunk, min(numel, (k + 1) * kEmaChunk)) of it, k = c - first[j].
__global__ __launch_bounds__(256) void ema_step_kernel(const dsg_ema_job* __restrict__ jobs, const int64_t* __restrict__ first,
                                                       int njobs, float omd) {
  const int64_t c = blockIdx.x;
  if (c >= first[njobs]) return;
  int lo = 0, hi = njobs;  // first[lo] <= c < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= c) lo = mid;
    else hi = mid;
  }
  const dsg_ema_job jb = jobs[lo];
  const int64_t base = (c - first[lo]) * kEmaChunk;
  if (base >= jb.numel) return;  // (a table whose chunk counts are too large for its jobs: nothing outside a job is touched)
  const int64_t left = jb.numel - base;
  const int n = left < kEmaChunk ? (int)left : kEmaChunk;  // elements of this chunk
  const gfloat* p = (const gfloat*)(jb.param + base);
  gfloat* s = (gfloat*)(jb.shadow + base);
  const bool copy_only = jb.copy_only != 0;
  const bool vec = ((reinterpret_cast<uintptr_t>(jb.param) | reinterpret_cast<uintptr_t>(jb.shadow)) & 15) == 0;
  const int tid = threadIdx.x;
  if (!vec) {  // dword path: either pointer off a 16-byte boundary
    for (int e = tid; e < n; e += 256) s[e] = copy_only ? p[e] : ema_elem(s[e], p[e], omd);
    return;
  }
  if (n == kEmaChunk) {  // a whole chunk (all but a job's last): every load is issued before the first use
    f32x4 pv[kEmaRows], sv[kEmaRows];
#pragma unroll
    for (int r = 0; r < kEmaRows; ++r) pv[r] = *(const gfloat4*)(p + (r * 256 + tid) * 4);
    if (!copy_only) {
#pragma unroll
      for (int r = 0; r < kEmaRows; ++r) sv[r] = *(const gfloat4*)(s + (r * 256 + tid) * 4);
#pragma unroll
      for (int r = 0; r < kEmaRows; ++r) pv[r] = ema_elem4(sv[r], pv[r], omd);
    }
#pragma unroll
    for (int r = 0; r < kEmaRows; ++r) *(gfloat4*)(s + (r * 256 + tid) * 4) = pv[r];
    return;
  }
  const int n4 = n & ~3;  // whole float4 groups; the numel % 4 tail goes one dword at a time
  for (int e = tid * 4; e < n4; e += 256 * 4) {
    const f32x4 pv = *(const gfloat4*)(p + e);
    *(gfloat4*)(s + e) = copy_only ? pv : ema_elem4(*(const gfloat4*)(s + e), pv, omd);
  }
  const int e = n4 + tid;
  if (e < n) s[e] = copy_only ? p[e] : ema_elem(s[e], p[e], omd);
}

}  // namespace dsg

// chunks of one job: THE chunk rule (the kernel, the Python wrapper and the tests take it from here)
DSG_API int dsg_ema_job_chunks(const dsg_ema_job* job, int64_t* chunks) {
  DSG_CHECK_ARG(job != nullptr && chunks != nullptr, "dsg_ema_job_chunks: NULL pointer");
  DSG_CHECK_ARG(job->param != nullptr && job->shadow != nullptr, "dsg_ema_job_chunks: NULL param or shadow");
  DSG_CHECK_ARG(job->numel > 0, "dsg_ema_job_chunks: numel must be positive");
  DSG_CHECK_ARG((reinterpret_cast<uintptr_t>(job->param) & 3) == 0 && (reinterpret_cast<uintptr_t>(job->shadow) & 3) == 0,
                "dsg_ema_job_chunks: pointers must be 4-byte aligned");
  *chunks = dsg::cdiv64(job->numel, dsg::kEmaChunk);
  return DSG_OK;
}

DSG_API int dsg_ema_step(const dsg_ema_job* jobs_dev, const int64_t* first_dev, int32_t njobs, int64_t total_chunks,
                         float one_minus_decay, void* stream) {
  DSG_CHECK_ARG(njobs >= 0, "dsg_ema_step: njobs=%d is negative", njobs);
  DSG_CHECK_ARG(one_minus_decay >= 0.f && one_minus_decay <= 1.f, "dsg_ema_step: one_minus_decay=%g is outside [0, 1]",
                (double)one_minus_decay);
  if (njobs == 0) return DSG_OK;
  DSG_CHECK_ARG(jobs_dev != nullptr && first_dev != nullptr, "dsg_ema_step: NULL job table");
  DSG_CHECK_ARG(total_chunks >= njobs, "dsg_ema_step: total_chunks=%lld for %d jobs (every job has at least one chunk)",
                (long long)total_chunks, njobs);
  DSG_CHECK_ARG(total_chunks <= 0x7FFFFFFF, "dsg_ema_step: too many chunks");
  hipLaunchKernelGGL(dsg::ema_step_kernel, dim3((unsigned)total_chunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     jobs_dev, first_dev, njobs, one_minus_decay);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}
