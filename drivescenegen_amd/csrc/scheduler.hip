// Noise-scheduler elementwise kernels for gfx950 (HBM-bound streaming, float4 per lane).
//
// Replaces the tensor arithmetic of diffusers' DDPMScheduler.add_noise / .step and
// DDIMScheduler.step (reference call sites: DriveSceneGen/pipeline/training_pipeline.py:80
// `noise_scheduler.add_noise`, and the DDPMPipeline loop behind training_pipeline.py:26-32 and
// DriveSceneGen/scripts/generation.py:14-20; formulas SURVEY.md App. A.3 / A.3b / A.4).
// Every expression is evaluated with individually rounded fp32 operations in the reference's
// order (fma contraction disabled for this file, IEEE division), so results are bit-identical to torch-CPU.
#include "dsg_common.h"

// HIP's __fmul_rn/__fadd_rn are plain operators (contractible); forbid fma contraction for this TU instead.
#pragma clang fp contract(off)

namespace dsg {

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// grid = (ceil(per_sample/1024), n)
__global__ __launch_bounds__(256) void add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ nz,
                                                        const float* __restrict__ sa, const float* __restrict__ sb,
                                                        float* __restrict__ out, int64_t per) {
  const int n = blockIdx.y;
  const float a = sa[n], b = sb[n];
  const int64_t base = (int64_t)n * per;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= per) return;
  if ((per & 3) == 0) {
    const float4 x = *reinterpret_cast<const float4*>(x0 + base + i0);
    const float4 e = *reinterpret_cast<const float4*>(nz + base + i0);
    float4 r;
    r.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, e.x));
    r.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, e.y));
    r.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, e.z));
    r.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, e.w));
    *reinterpret_cast<float4*>(out + base + i0) = r;
  } else {
    for (int k = 0; k < 4 && i0 + k < per; ++k)
      out[base + i0 + k] = __fadd_rn(__fmul_rn(a, x0[base + i0 + k]), __fmul_rn(b, nz[base + i0 + k]));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Counter-based device noise (opt-in replacement of the training loop's HOST draw, training_pipeline.py:72
// `torch.randn(batch.shape).to(device)`: 500 ms of one CPU thread for configs[4]'s [128, 8, 256, 256] against a 183-ms
// GPU step).  Philox4x32-10 (Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
// Random123 known-answer vectors are in tests/test_oracle_kat.py) + Box-Muller.  THE STREAM IS DEFINED BY THIS TEXT and
// restated in oracle/philox_oracle.py:
//   element e of the flat tensor takes lane e % 4 of the block  Philox4x32-10(counter = (c.lo, c.hi, offset.lo, offset.hi),
//   key = (seed.lo, seed.hi)),  c = e / 4;  lanes (0, 1) and (2, 3) are Box-Muller pairs:
//     u1 = (float(r_even) + 0.5f) * 2^-32     in (0, 1]   (uint32 -> fp32 round-to-nearest-even; never 0: no log(0))
//     u2 =  float(r_odd)          * 2^-32     in [0, 1]
//     rad = sqrtf(-2 * logf(u1));   z_even = rad * cospif(2 * u2);   z_odd = rad * sinpif(2 * u2)
// A (seed, offset) pair names one tensor; the caller advances `offset` per draw (the training loop: its step counter, the
// rank in the high bits) -- no state lives on the device.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& za, float& zb) {
  const float u1 = __fmul_rn(__fadd_rn((float)ra, 0.5f), 0x1p-32f);
  const float u2 = __fmul_rn((float)rb, 0x1p-32f);
  const float rad = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  const float th = __fmul_rn(2.0f, u2);
  za = __fmul_rn(rad, cospif(th));
  zb = __fmul_rn(rad, sinpif(th));
}

// MODE 0: raw uint32 blocks (tests, and a general counter-based generator);  1: z ~ N(0,1) -> noise;
// 2: z -> noise AND noisy = sa[n]*x0 + sb[n]*z in the same pass (add_noise_kernel's two-multiply-one-add, bit for bit)
template <int MODE>
__global__ __launch_bounds__(256) void philox_kernel(const float* __restrict__ x0, const float* __restrict__ sa,
                                                     const float* __restrict__ sb, float* __restrict__ noisy,
                                                     void* __restrict__ noise_out, int64_t numel, int64_t per,
                                                     uint32_t seed_lo, uint32_t seed_hi, uint32_t off_lo, uint32_t off_hi) {
  const int64_t blocks = (numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool vec = (numel & 3) == 0 && (per & 3) == 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < blocks; c += stride) {
    uint32_t r[4];
    philox4x32_10((uint32_t)c, (uint32_t)((uint64_t)c >> 32), off_lo, off_hi, seed_lo, seed_hi, r);
    const int64_t e = c << 2;
    if (MODE == 0) {
      uint32_t* o = reinterpret_cast<uint32_t*>(noise_out);
      if ((numel & 3) == 0) {
        *reinterpret_cast<uint4*>(o + e) = make_uint4(r[0], r[1], r[2], r[3]);
      } else {
        for (int k = 0; k < 4 && e + k < numel; ++k) o[e + k] = r[k];
      }
      continue;
    }
    float z[4];
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
    float* o = reinterpret_cast<float*>(noise_out);
    if (vec) {
      *reinterpret_cast<float4*>(o + e) = make_float4(z[0], z[1], z[2], z[3]);
      if (MODE == 2) {
        const int64_t n = e / per;
        const float a = sa[n], b = sb[n];
        const float4 x = *reinterpret_cast<const float4*>(x0 + e);
        float4 q;
        q.x = __fadd_rn(__fmul_rn(a, x.x), __fmul_rn(b, z[0]));
        q.y = __fadd_rn(__fmul_rn(a, x.y), __fmul_rn(b, z[1]));
        q.z = __fadd_rn(__fmul_rn(a, x.z), __fmul_rn(b, z[2]));
        q.w = __fadd_rn(__fmul_rn(a, x.w), __fmul_rn(b, z[3]));
        *reinterpret_cast<float4*>(noisy + e) = q;
      }
    } else {
      for (int k = 0; k < 4 && e + k < numel; ++k) {
        o[e + k] = z[k];
        if (MODE == 2) {
          const int64_t n = (e + k) / per;
          noisy[e + k] = __fadd_rn(__fmul_rn(sa[n], x0[e + k]), __fmul_rn(sb[n], z[k]));
        }
      }
    }
  }
}

__device__ __forceinline__ float pred_x0(float x, float e, float sb, float sa, float clip) {
  float v = __fdiv_rn(__fsub_rn(x, __fmul_rn(sb, e)), sa);
  if (clip > 0.f) v = clampf(v, -clip, clip);
  return v;
}

__global__ __launch_bounds__(256) void ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                        const float* __restrict__ nz, float* __restrict__ prev,
                                                        int64_t numel, float sb, float sa, float clip, float c0,
                                                        float ct, float sigma) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const float xv = x[i];
    const float p0 = pred_x0(xv, eps[i], sb, sa, clip);
    float r = __fadd_rn(__fmul_rn(c0, p0), __fmul_rn(ct, xv));
    if (nz) r = __fadd_rn(r, __fmul_rn(sigma, nz[i]));
    prev[i] = r;
  }
}

__global__ __launch_bounds__(256) void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                        float* __restrict__ prev, int64_t numel, float sb, float sa,
                                                        float clip, float sap, float dc) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const float e = eps[i];
    const float p0 = pred_x0(x[i], e, sb, sa, clip);
    prev[i] = __fadd_rn(__fmul_rn(sap, p0), __fmul_rn(dc, e));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// RePaint (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers' RePaintScheduler.step / .undo_step): scene completion with an
// unconditional network.  One pass per reverse step, per element and in THIS order (include/dsg.h states it as the contract):
//   p0      = (x - sb*e) / sa, clamped to +-clip when clip > 0                 (pred_x0 above)
//   unknown = sap*p0 + dc*e     [+ std*z  when add_std]
//   known   = sap*orig + sbp*z
//   prev    = m*known + (1 - m)*unknown
// z is ONE noise value per element, used in both places: read from `nz` (device memory or a pinned host buffer, SRC 0) or made
// here from the Philox stream above (SRC 1: element e = lane e % 4 of block e / 4, dsg_philox_normal's mapping).  Each lane
// owns one Philox block = 4 consecutive elements; with hw % 4 == 0 and 16-byte aligned pointers (VEC) those share (n, c), so
// every stream is one dwordx4 access and `orig` / `m` are addressed through their batch / channel strides (0 = broadcast).
struct repaint_geom {
  int64_t numel, chw, hw;
  int64_t orig_sn;          // 0 (one original for the batch) or chw
  int64_t m_sn, m_sc;       // mask strides over n and c: 0 where its extent is 1
};

__device__ __forceinline__ float repaint_elem(float x, float e, float o, float m, float z, float sb, float sa, float clip,
                                              float sap, float dc, float sd, float sbp, bool add_std) {
  const float p0 = pred_x0(x, e, sb, sa, clip);
  float unknown = __fadd_rn(__fmul_rn(sap, p0), __fmul_rn(dc, e));
  if (add_std) unknown = __fadd_rn(unknown, __fmul_rn(sd, z));
  // (the empty asm pins this product in a register of its own: hipcc otherwise pairs it with sbp*z into v_pk_mul_f32 and sums
  //  the pair with v_pk_add_f32 ... op_sel:[0,1], the form tests/test_isa_policy.py bans; same arithmetic, same rounding)
  float ko = __fmul_rn(sap, o);
  asm volatile("" : "+v"(ko));
  const float known = __fadd_rn(ko, __fmul_rn(sbp, z));
  return __fadd_rn(__fmul_rn(m, known), __fmul_rn(__fsub_rn(1.0f, m), unknown));
}

template <int SRC>
__device__ __forceinline__ void repaint_noise4(const float* nz, int64_t c, int64_t numel, bool vec, uint32_t seed_lo,
                                               uint32_t seed_hi, uint32_t off_lo, uint32_t off_hi, float (&z)[4]) {
  const int64_t e = c << 2;
  if (SRC == 0) {
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(nz + e);
      z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
      for (int k = 0; k < 4; ++k) z[k] = e + k < numel ? nz[e + k] : 0.f;
    }
  } else {
    uint32_t r[4];
    philox4x32_10((uint32_t)c, (uint32_t)((uint64_t)c >> 32), off_lo, off_hi, seed_lo, seed_hi, r);
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
  }
}

template <int SRC, bool VEC>
__global__ __launch_bounds__(256) void repaint_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                           const float* __restrict__ orig, const float* __restrict__ mask,
                                                           const float* __restrict__ nz, float* __restrict__ prev,
                                                           float* __restrict__ noise_out, repaint_geom g, float sb, float sa,
                                                           float clip, float sap, float dc, float sd, float sbp, int add_std,
                                                           uint32_t seed_lo, uint32_t seed_hi, uint32_t off_lo,
                                                           uint32_t off_hi) {
  const int64_t blocks = (g.numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool sdz = add_std != 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < blocks; c += stride) {
    float z[4];
    repaint_noise4<SRC>(nz, c, g.numel, VEC, seed_lo, seed_hi, off_lo, off_hi, z);
    const int64_t e = c << 2;
    if (VEC) {
      const int64_t n = e / g.chw, rem = e - n * g.chw;
      const int64_t ch = rem / g.hw, p = rem - ch * g.hw;
      const float4 xv = *reinterpret_cast<const float4*>(x + e);
      const float4 ev = *reinterpret_cast<const float4*>(eps + e);
      const float4 ov = *reinterpret_cast<const float4*>(orig + n * g.orig_sn + rem);
      const float4 mv = *reinterpret_cast<const float4*>(mask + n * g.m_sn + ch * g.m_sc + p);
      float4 r;
      r.x = repaint_elem(xv.x, ev.x, ov.x, mv.x, z[0], sb, sa, clip, sap, dc, sd, sbp, sdz);
      r.y = repaint_elem(xv.y, ev.y, ov.y, mv.y, z[1], sb, sa, clip, sap, dc, sd, sbp, sdz);
      r.z = repaint_elem(xv.z, ev.z, ov.z, mv.z, z[2], sb, sa, clip, sap, dc, sd, sbp, sdz);
      r.w = repaint_elem(xv.w, ev.w, ov.w, mv.w, z[3], sb, sa, clip, sap, dc, sd, sbp, sdz);
      *reinterpret_cast<float4*>(prev + e) = r;
      if (noise_out) *reinterpret_cast<float4*>(noise_out + e) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
      for (int k = 0; k < 4 && e + k < g.numel; ++k) {
        const int64_t i = e + k;
        const int64_t n = i / g.chw, rem = i - n * g.chw;
        const int64_t ch = rem / g.hw, p = rem - ch * g.hw;
        prev[i] = repaint_elem(x[i], eps[i], orig[n * g.orig_sn + rem], mask[n * g.m_sn + ch * g.m_sc + p], z[k], sb, sa,
                               clip, sap, dc, sd, sbp, sdz);
        if (noise_out) noise_out[i] = z[k];
      }
    }
  }
}

// RePaint's jump back in time (one forward-diffusion step): out = ck*x + cz*z, z as above
template <int SRC, bool VEC>
__global__ __launch_bounds__(256) void repaint_undo_kernel(const float* __restrict__ x, const float* __restrict__ nz,
                                                           float* __restrict__ out, int64_t numel, float ck, float cz,
                                                           uint32_t seed_lo, uint32_t seed_hi, uint32_t off_lo,
                                                           uint32_t off_hi) {
  const int64_t blocks = (numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < blocks; c += stride) {
    float z[4];
    repaint_noise4<SRC>(nz, c, numel, VEC, seed_lo, seed_hi, off_lo, off_hi, z);
    const int64_t e = c << 2;
    if (VEC) {
      const float4 xv = *reinterpret_cast<const float4*>(x + e);
      float4 r;
      r.x = __fadd_rn(__fmul_rn(ck, xv.x), __fmul_rn(cz, z[0]));
      r.y = __fadd_rn(__fmul_rn(ck, xv.y), __fmul_rn(cz, z[1]));
      r.z = __fadd_rn(__fmul_rn(ck, xv.z), __fmul_rn(cz, z[2]));
      r.w = __fadd_rn(__fmul_rn(ck, xv.w), __fmul_rn(cz, z[3]));
      *reinterpret_cast<float4*>(out + e) = r;
    } else {
      for (int k = 0; k < 4 && e + k < numel; ++k) out[e + k] = __fadd_rn(__fmul_rn(ck, x[e + k]), __fmul_rn(cz, z[k]));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// DPM-Solver++ multistep (Lu et al., 2022; diffusers' DPMSolverMultistepScheduler.step): the data-prediction form of the
// diffusion ODE's exponential integrator, orders 1-3, and its SDE variant.  One pass per step, per element and in THIS order
// (include/dsg.h states it as the contract):
//   m0   = (x - sigma_s*e) / alpha_s                      -> m0_out (the history entry this step adds)
//   D10  = inv_r0*(m0 - m1)                               ORDER >= 2
//   D11  = inv_r1*(m1 - m2);  dd = D10 - D11;  D1 = D10 + q*dd;  D2 = p*dd        ORDER == 3 (D1 = D10 at order 2)
//   prev = kx*x + c0*m0  [+ c1*D1]  [+ c2*D2]  [+ cn*z]   summed left to right
// The host passes signed coefficients.  z as in repaint_step_kernel (NOISE 1: read from `nz`, 2: this lane's Philox block;
// 0: no noise term).  VEC: every pointer is 16-byte aligned, so a lane's 4 elements are one dwordx4 access per stream; the last
// numel % 4 elements take the per-element path, as everything does without VEC.
struct dpm_coef {
  float sigma_s, alpha_s, inv_r0, inv_r1, q, p, kx, c0, c1, c2, cn;
};

template <int ORDER, bool NOISE>
__device__ __forceinline__ void dpm_elem(float x, float e, float m1, float m2, float z, const dpm_coef& k, float& prev,
                                         float& m0o) {
  const float m0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(k.sigma_s, e)), k.alpha_s);
  float r = __fadd_rn(__fmul_rn(k.kx, x), __fmul_rn(k.c0, m0));
  if (ORDER >= 2) {
    const float d10 = __fmul_rn(k.inv_r0, __fsub_rn(m0, m1));
    float d1 = d10;
    if (ORDER == 3) {
      const float d11 = __fmul_rn(k.inv_r1, __fsub_rn(m1, m2));
      const float dd = __fsub_rn(d10, d11);
      d1 = __fadd_rn(d10, __fmul_rn(k.q, dd));
      r = __fadd_rn(r, __fmul_rn(k.c1, d1));
      r = __fadd_rn(r, __fmul_rn(k.c2, __fmul_rn(k.p, dd)));
    } else {
      r = __fadd_rn(r, __fmul_rn(k.c1, d1));
    }
  }
  if (NOISE) r = __fadd_rn(r, __fmul_rn(k.cn, z));
  prev = r;
  m0o = m0;
}

template <int ORDER, int NOISE, bool VEC>
__global__ __launch_bounds__(256) void dpmsolver_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                             const float* __restrict__ m1, const float* __restrict__ m2,
                                                             const float* __restrict__ nz, float* __restrict__ prev,
                                                             float* __restrict__ m0_out, float* __restrict__ noise_out,
                                                             int64_t numel, dpm_coef k, uint32_t seed_lo, uint32_t seed_hi,
                                                             uint32_t off_lo, uint32_t off_hi) {
  const int64_t blocks = (numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < blocks; c += stride) {
    const int64_t e = c << 2;
    const bool vec = VEC && e + 4 <= numel;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (NOISE == 1) repaint_noise4<0>(nz, c, numel, vec, seed_lo, seed_hi, off_lo, off_hi, z);
    if (NOISE == 2) repaint_noise4<1>(nz, c, numel, vec, seed_lo, seed_hi, off_lo, off_hi, z);
    if (vec) {
      const float4 xv = *reinterpret_cast<const float4*>(x + e);
      const float4 ev = *reinterpret_cast<const float4*>(eps + e);
      float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av, r, m;
      if (ORDER >= 2) av = *reinterpret_cast<const float4*>(m1 + e);
      if (ORDER == 3) bv = *reinterpret_cast<const float4*>(m2 + e);
      dpm_elem<ORDER, NOISE != 0>(xv.x, ev.x, av.x, bv.x, z[0], k, r.x, m.x);
      dpm_elem<ORDER, NOISE != 0>(xv.y, ev.y, av.y, bv.y, z[1], k, r.y, m.y);
      dpm_elem<ORDER, NOISE != 0>(xv.z, ev.z, av.z, bv.z, z[2], k, r.z, m.z);
      dpm_elem<ORDER, NOISE != 0>(xv.w, ev.w, av.w, bv.w, z[3], k, r.w, m.w);
      *reinterpret_cast<float4*>(prev + e) = r;
      *reinterpret_cast<float4*>(m0_out + e) = m;
      if (NOISE != 0 && noise_out) *reinterpret_cast<float4*>(noise_out + e) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
      for (int j = 0; j < 4 && e + j < numel; ++j) {
        const int64_t i = e + j;
        float r, m;
        dpm_elem<ORDER, NOISE != 0>(x[i], eps[i], ORDER >= 2 ? m1[i] : 0.f, ORDER == 3 ? m2[i] : 0.f, z[j], k, r, m);
        prev[i] = r;
        m0_out[i] = m;
        if (NOISE != 0 && noise_out) noise_out[i] = z[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Dynamic thresholding (Saharia et al., "Imagen", 2022, section 2.3; diffusers 0.20.0 `_threshold_sample`): per sample, the
// q-quantile of |p0| -- torch.quantile's linear interpolation between two neighbouring order statistics -- clamped into
// [1, sample_max_value] is the scale s[n]; the step then uses clamp(p0, -s, s) / s in place of the statically clipped p0
// (include/dsg.h states the arithmetic as the contract).  p0 is never stored: every pass recomputes it with pred_x0, the
// function the step kernels use, so the bits agree.
//
// The two order statistics come from an exact MSB-first radix select on key = bits(|p0|) (sign bit clear: the pattern orders
// like the value for everything that is no NaN; NaN patterns sort last and are counted apart), 11 + 11 + 9 bits:
//   thr_hist_kernel<P>   every element whose key starts with the prefix chosen so far counts its next digit into a per-block LDS
//                        histogram, which is flushed (non-zero bins) with integer atomics into the sample's global histogram;
//   thr_scan_kernel<P>   one block per sample: finds the digit that holds each of the two ranks, extends the two prefixes,
//                        rebases the two ranks, zeroes the histograms for the next pass; after the last pass the prefixes ARE
//                        v_lo and v_hi, and it writes s[n].
// The two ranks are neighbours (k_hi - k_lo <= 1) but may fall into different bins: from then on there are two prefixes and two
// histograms.  While the prefixes agree only histogram 0 is kept.  Integer counts: the result does not depend on arrival order.
// No loop here depends on the data, so NaN / Inf keys cannot keep a kernel from ending.
// Workspace per sample (32-bit words): THR_STATE state words, then two histograms of THR_BINS.
constexpr int THR_BINS = 2048;
constexpr int THR_STATE = 16;      // [0] prefix_lo [1] prefix_hi [2] rank_lo [3] rank_hi [4] NaN seen
constexpr int THR_WORDS = THR_STATE + 2 * THR_BINS;

template <int PASS> struct thr_digit;
template <> struct thr_digit<1> { static constexpr int shift = 20, bins = 2048, prefix_shift = 31; };
template <> struct thr_digit<2> { static constexpr int shift = 9, bins = 2048, prefix_shift = 20; };
template <> struct thr_digit<3> { static constexpr int shift = 0, bins = 512, prefix_shift = 9; };

// One count per lane with `valid` into h[bin].  Called by all 64 lanes of a wave together.  When every valid lane names the same
// bin (an all-equal row; real rasters, whose values sit in a few exponent bins, often) ONE lane adds the lane count: the LDS
// atomic unit would otherwise serve the 64 adds to one address one after another.
__device__ __forceinline__ void thr_count(uint32_t* h, uint32_t bin, bool valid) {
  const unsigned long long m = __ballot(valid);
  if (m == 0) return;
  const int lead = __ffsll(m) - 1;
  const uint32_t first = (uint32_t)__shfl((int)bin, lead);
  if (__ballot(valid && bin != first) == 0) {
    if ((int)(threadIdx.x & 63) == lead) atomicAdd(&h[first], (uint32_t)__popcll(m));
  } else if (valid) {
    atomicAdd(&h[bin], 1u);
  }
}

template <int PASS>
__device__ __forceinline__ void thr_count_key(uint32_t* h, uint32_t key, bool valid, uint32_t pfx_lo, uint32_t pfx_hi, bool two) {
  typedef thr_digit<PASS> D;
  const uint32_t bin = (key >> D::shift) & (uint32_t)(D::bins - 1);
  if (PASS == 1) {
    thr_count(h, bin, valid);
  } else {
    const uint32_t head = key >> D::prefix_shift;
    thr_count(h, bin, valid && head == pfx_lo);
    if (two) thr_count(h + THR_BINS, bin, valid && head == pfx_hi);      // (`two` is the same in every lane of the grid row)
  }
}

// grid = (blocks per sample, n); a block walks its share of the sample's `per` elements 1024 at a time, 4 consecutive per lane
template <int PASS, bool VEC>
__global__ __launch_bounds__(256) void thr_hist_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                       uint32_t* __restrict__ ws, int64_t per, float sb, float sa) {
  typedef thr_digit<PASS> D;
  __shared__ uint32_t h[2 * THR_BINS];
  __shared__ uint32_t nan_seen;
  uint32_t* st = ws + (int64_t)blockIdx.y * THR_WORDS;
  const uint32_t pfx_lo = PASS == 1 ? 0u : st[0], pfx_hi = PASS == 1 ? 0u : st[1];
  const bool two = PASS != 1 && pfx_lo != pfx_hi;
  for (int b = threadIdx.x; b < (two ? 2 : 1) * THR_BINS; b += 256) h[b] = 0;
  if (threadIdx.x == 0) nan_seen = 0;
  __syncthreads();
  const float* xr = x + (int64_t)blockIdx.y * per;
  const float* er = eps + (int64_t)blockIdx.y * per;
  bool nan = false;
  const int64_t stride = (int64_t)gridDim.x * 1024;
  for (int64_t base = (int64_t)blockIdx.x * 1024; base < per; base += stride) {     // (the same trip count in every lane)
    const int64_t i0 = base + (int64_t)threadIdx.x * 4;
    float xv[4], ev[4];
    if (VEC && i0 + 4 <= per) {
      const float4 a = *reinterpret_cast<const float4*>(xr + i0);
      const float4 c = *reinterpret_cast<const float4*>(er + i0);
      xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w;
      ev[0] = c.x; ev[1] = c.y; ev[2] = c.z; ev[3] = c.w;
    } else {
      for (int j = 0; j < 4; ++j) {
        const bool in = i0 + j < per;
        xv[j] = in ? xr[i0 + j] : 0.f;
        ev[j] = in ? er[i0 + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t key = __float_as_uint(pred_x0(xv[j], ev[j], sb, sa, 0.f)) & 0x7fffffffu;
      const bool valid = i0 + j < per;
      if (PASS == 1) nan = nan || (valid && key > 0x7f800000u);
      thr_count_key<PASS>(h, key, valid, pfx_lo, pfx_hi, two);
    }
  }
  if (PASS == 1 && nan) nan_seen = 1;        // (a benign race: every writer stores 1)
  __syncthreads();
  uint32_t* g = st + THR_STATE;
  for (int b = threadIdx.x; b < D::bins; b += 256) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&g[b], c);
    if (two) {
      const uint32_t c1 = h[THR_BINS + b];
      if (c1) atomicAdd(&g[THR_BINS + b], c1);
    }
  }
  if (PASS == 1 && threadIdx.x == 0 && nan_seen) atomicOr(&st[4], 1u);
}

// grid = n, 256 threads; thread t owns bins [t*PER, (t+1)*PER) of both histograms
template <int PASS>
__global__ __launch_bounds__(256) void thr_scan_kernel(uint32_t* __restrict__ ws, float* __restrict__ s_out, uint32_t k_lo,
                                                       uint32_t k_hi, float w, float max_value) {
  typedef thr_digit<PASS> D;
  constexpr int PER = D::bins / 256;
  __shared__ uint32_t part[256];
  __shared__ uint32_t found[4];         // digit_lo, rank_lo', digit_hi, rank_hi'
  uint32_t* st = ws + (int64_t)blockIdx.x * THR_WORDS;
  uint32_t* g = st + THR_STATE;
  const uint32_t pfx[2] = {PASS == 1 ? 0u : st[0], PASS == 1 ? 0u : st[1]};
  const uint32_t rank[2] = {PASS == 1 ? k_lo : st[2], PASS == 1 ? k_hi : st[3]};
  const bool two = PASS != 1 && pfx[0] != pfx[1];
  const int t = threadIdx.x;
  if (t < 4) found[t] = 0;              // (a histogram that does not hold the rank -- a caller's broken workspace -- gives digit 0)
  for (int which = 0; which < 2; ++which) {
    const uint32_t* hist = g + (which == 1 && two ? THR_BINS : 0);
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { c[j] = hist[t * PER + j]; sum += c[j]; }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {            // inclusive scan of the 256 partial sums
      const uint32_t add = t >= d ? part[t - d] : 0u;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    uint32_t before = part[t] - sum;               // elements in the bins below this thread's
    const uint32_t r = rank[which];
    if (r >= before && r - before < sum) {         // exactly one thread: the counts sum to more than r
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (r >= before && r - before < c[j]) {
          found[2 * which] = (uint32_t)(t * PER + j);
          found[2 * which + 1] = r - before;
        }
        before += c[j];
      }
    }
    __syncthreads();
  }
  // the histograms are read: zero them for the next pass (each thread its own bins, which nobody else read)
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    g[t * PER + j] = 0;
    if (two) g[THR_BINS + t * PER + j] = 0;
  }
  if (t == 0) {
    const uint32_t v_lo = (pfx[0] << (D::prefix_shift - D::shift)) | found[0];
    const uint32_t v_hi = (pfx[1] << (D::prefix_shift - D::shift)) | found[2];
    if (PASS < 3) {
      st[0] = v_lo; st[1] = v_hi; st[2] = found[1]; st[3] = found[3];
    } else {
      const float lo = __uint_as_float(v_lo), hi = __uint_as_float(v_hi);
      const float d = __fsub_rn(hi, lo);
      const float quant = w < 0.5f ? fmaf(w, d, lo) : fmaf(-d, __fsub_rn(1.0f, w), hi);      // torch.lerp, bit for bit
      float s = fminf(fmaxf(quant, 1.0f), max_value);
      if (st[4] != 0 || quant != quant) s = __uint_as_float(0x7fc00000u);       // a NaN in the row: torch.quantile's answer
      s_out[blockIdx.x] = s;
    }
  }
}

// p0 clamped to +-s and divided by s (IEEE division): the thresholded data prediction
__device__ __forceinline__ float thr_x0(float x, float e, float sb, float sa, float s) {
  return __fdiv_rn(clampf(pred_x0(x, e, sb, sa, 0.f), -s, s), s);
}

// The scales of the (up to) 4 consecutive elements from flat index e on: one division when they share a sample
__device__ __forceinline__ void thr_scales4(const float* __restrict__ thr, int64_t e, int64_t per, float (&s)[4]) {
  const int64_t n = e / per, rem = e - n * per;
  if (rem + 4 <= per) {
    s[0] = s[1] = s[2] = s[3] = thr[n];
  } else {                                          // the quad crosses into the next sample(s): per % 4 != 0 only
    for (int j = 0; j < 4; ++j) s[j] = thr[(e + j) / per];
  }
}

// MODE 0: DDPM (prev = c0*x0' + ct*x [+ sigma*z]), a = c0, b = ct, c = sigma;  1: DDIM (prev = sap*x0' + dc*e), a = sap, b = dc
template <int MODE>
__device__ __forceinline__ float thr_step_elem(float x, float e, float z, bool add_z, float s, float sb, float sa, float a, float b,
                                               float c) {
  const float p0 = thr_x0(x, e, sb, sa, s);
  if (MODE == 1) return __fadd_rn(__fmul_rn(a, p0), __fmul_rn(b, e));
  float r = __fadd_rn(__fmul_rn(a, p0), __fmul_rn(b, x));
  if (add_z) r = __fadd_rn(r, __fmul_rn(c, z));
  return r;
}

// One lane = 4 consecutive elements; VEC: every pointer is 16-byte aligned, so they move as one dwordx4 per stream; the last
// numel % 4 elements take the per-element path, as everything does without VEC.  thr is read at index < numel / per only.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void thr_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                       const float* __restrict__ nz, const float* __restrict__ thr,
                                                       float* __restrict__ prev, int64_t numel, int64_t per, float sb, float sa,
                                                       float a, float b, float c) {
  const int64_t quads = (numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool add_z = MODE == 0 && nz != nullptr;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) {
    const int64_t e = q << 2;
    if (VEC && e + 4 <= numel) {
      float s[4];
      thr_scales4(thr, e, per, s);
      const float4 xv = *reinterpret_cast<const float4*>(x + e);
      const float4 ev = *reinterpret_cast<const float4*>(eps + e);
      float4 zv = make_float4(0.f, 0.f, 0.f, 0.f), r;
      if (add_z) zv = *reinterpret_cast<const float4*>(nz + e);
      r.x = thr_step_elem<MODE>(xv.x, ev.x, zv.x, add_z, s[0], sb, sa, a, b, c);
      r.y = thr_step_elem<MODE>(xv.y, ev.y, zv.y, add_z, s[1], sb, sa, a, b, c);
      r.z = thr_step_elem<MODE>(xv.z, ev.z, zv.z, add_z, s[2], sb, sa, a, b, c);
      r.w = thr_step_elem<MODE>(xv.w, ev.w, zv.w, add_z, s[3], sb, sa, a, b, c);
      *reinterpret_cast<float4*>(prev + e) = r;
    } else {
      for (int j = 0; j < 4 && e + j < numel; ++j) {
        const int64_t i = e + j;
        prev[i] = thr_step_elem<MODE>(x[i], eps[i], add_z ? nz[i] : 0.f, add_z, thr[i / per], sb, sa, a, b, c);
      }
    }
  }
}

// (x/2 + 0.5).clamp(0,1), NCHW -> NHWC.  grid = (ceil(hw/256), n)
template <int MODE>
__global__ __launch_bounds__(256) void postprocess_kernel(const float* __restrict__ x, void* __restrict__ out, int c,
                                                          int hw) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  for (int ci = 0; ci < c; ++ci) {
    float v = x[((size_t)n * c + ci) * hw + p];
    v = clampf(__fadd_rn(__fdiv_rn(v, 2.0f), 0.5f), 0.f, 1.f);
    const size_t o = ((size_t)n * hw + p) * c + ci;
    if (MODE == 0) {
      reinterpret_cast<float*>(out)[o] = v;
    } else if (MODE == 1) {
      reinterpret_cast<uint8_t*>(out)[o] = (uint8_t)rintf(__fmul_rn(v, 255.0f));
    } else {
      reinterpret_cast<uint8_t*>(out)[o] = (uint8_t)__fmul_rn(v, 255.0f);
    }
  }
}

static inline int stream_blocks(int64_t numel) {
  int64_t b = cdiv64(numel, 256);
  return (int)(b < 1 ? 1 : (b > 256 * 16 ? 256 * 16 : b));
}

}  // namespace dsg

DSG_API int dsg_add_noise(const float* x0, const float* noise, const float* sqrt_a, const float* sqrt_1ma, float* out,
                          int32_t n, int64_t per_sample, void* stream) {
  DSG_CHECK_ARG(x0 && noise && sqrt_a && sqrt_1ma && out, "dsg_add_noise: NULL pointer");
  DSG_CHECK_ARG(n > 0 && per_sample > 0 && n <= 65535, "dsg_add_noise: bad dims");
  hipLaunchKernelGGL(dsg::add_noise_kernel, dim3((unsigned)dsg::cdiv64(per_sample, 1024), n), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x0, noise, sqrt_a, sqrt_1ma, out, per_sample);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_ddpm_step(const float* sample, const float* eps, const float* noise, float* prev, int64_t numel,
                          float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float clip, float coef_x0, float coef_xt,
                          float sigma, void* stream) {
  DSG_CHECK_ARG(sample && eps && prev, "dsg_ddpm_step: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_ddpm_step: numel must be positive");
  hipLaunchKernelGGL(dsg::ddpm_step_kernel, dim3(dsg::stream_blocks(numel)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), sample, eps, noise, prev, numel, sqrt_beta_prod_t,
                     sqrt_alpha_prod_t, clip, coef_x0, coef_xt, sigma);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_ddim_step(const float* sample, const float* eps, float* prev, int64_t numel, float sqrt_beta_prod_t,
                          float sqrt_alpha_prod_t, float clip, float sqrt_alpha_prev, float dir_coef, void* stream) {
  DSG_CHECK_ARG(sample && eps && prev, "dsg_ddim_step: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_ddim_step: numel must be positive");
  hipLaunchKernelGGL(dsg::ddim_step_kernel, dim3(dsg::stream_blocks(numel)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), sample, eps, prev, numel, sqrt_beta_prod_t, sqrt_alpha_prod_t,
                     clip, sqrt_alpha_prev, dir_coef);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_postprocess(const float* x, void* out, int32_t n, int32_t c, int32_t hw, int32_t mode, void* stream) {
  DSG_CHECK_ARG(x && out, "dsg_postprocess: NULL pointer");
  DSG_CHECK_ARG(n > 0 && c > 0 && hw > 0 && n <= 65535, "dsg_postprocess: bad dims");
  DSG_CHECK_ARG(mode >= 0 && mode <= 2, "dsg_postprocess: mode must be 0, 1 or 2");
  dim3 grid(dsg::cdiv(hw, 256), n);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == 0) hipLaunchKernelGGL(dsg::postprocess_kernel<0>, grid, dim3(256), 0, st, x, out, c, hw);
  else if (mode == 1) hipLaunchKernelGGL(dsg::postprocess_kernel<1>, grid, dim3(256), 0, st, x, out, c, hw);
  else hipLaunchKernelGGL(dsg::postprocess_kernel<2>, grid, dim3(256), 0, st, x, out, c, hw);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
static inline int philox_blocks(int64_t numel) {
  int64_t b = cdiv64(cdiv64(numel, 4), 256);
  return (int)(b < 1 ? 1 : (b > 256 * 32 ? 256 * 32 : b));
}
}  // namespace dsg

DSG_API int dsg_philox_u32(uint32_t* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(out, "dsg_philox_u32: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_philox_u32: numel must be positive");
  hipLaunchKernelGGL(dsg::philox_kernel<0>, dim3(dsg::philox_blocks(numel)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (void*)out, numel,
                     (int64_t)4, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32));
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_philox_normal(float* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(out, "dsg_philox_normal: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_philox_normal: numel must be positive");
  hipLaunchKernelGGL(dsg::philox_kernel<1>, dim3(dsg::philox_blocks(numel)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, (void*)out, numel,
                     (int64_t)4, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32));
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_add_noise_philox(const float* x0, const float* sqrt_a, const float* sqrt_1ma, float* noisy, float* noise,
                                 int32_t n, int64_t per_sample, uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(x0 && sqrt_a && sqrt_1ma && noisy && noise, "dsg_add_noise_philox: NULL pointer");
  DSG_CHECK_ARG(n > 0 && per_sample > 0, "dsg_add_noise_philox: bad dims");
  const int64_t numel = (int64_t)n * per_sample;
  hipLaunchKernelGGL(dsg::philox_kernel<2>, dim3(dsg::philox_blocks(numel)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     x0, sqrt_a, sqrt_1ma, noisy, (void*)noise, numel, per_sample, (uint32_t)seed, (uint32_t)(seed >> 32),
                     (uint32_t)offset, (uint32_t)(offset >> 32));
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// do [a, a + abytes) and [b, b + bbytes) share a byte?  (NULL overlaps nothing)
static inline bool overlaps2(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y ? y - x < abytes : x - y < bbytes;
}

template <int PASS>
static void thr_pass(const float* x, const float* e, uint32_t* ws, float* s, int32_t n, int64_t per, float sb, float sa,
                     uint32_t k_lo, uint32_t k_hi, float w, float max_value, bool vec, hipStream_t st) {
  // enough blocks per sample to fill the chip at any batch, never more than the sample has 1024-element chunks
  int64_t bps = cdiv64(per, 1024), cap = cdiv64(2048, n);
  if (bps > cap) bps = cap;
  const dim3 grid((unsigned)bps, (unsigned)n), block(256);
  if (vec) hipLaunchKernelGGL((thr_hist_kernel<PASS, true>), grid, block, 0, st, x, e, ws, per, sb, sa);
  else hipLaunchKernelGGL((thr_hist_kernel<PASS, false>), grid, block, 0, st, x, e, ws, per, sb, sa);
  hipLaunchKernelGGL((thr_scan_kernel<PASS>), dim3((unsigned)n), block, 0, st, ws, s, k_lo, k_hi, w, max_value);
}
}  // namespace dsg

DSG_API int dsg_dynthresh_workspace_bytes(int32_t n, size_t* bytes) {
  DSG_CHECK_ARG(bytes, "dsg_dynthresh_workspace_bytes: NULL pointer");
  DSG_CHECK_ARG(n > 0 && n <= 65535, "dsg_dynthresh_workspace_bytes: n=%d outside [1, 65535]", n);
  *bytes = (size_t)n * dsg::THR_WORDS * sizeof(uint32_t);
  return DSG_OK;
}

DSG_API int dsg_dynthresh_scale(const float* sample, const float* eps, float* s, int32_t n, int64_t per_sample,
                                float sqrt_beta_prod_t, float sqrt_alpha_prod_t, int64_t k_lo, int64_t k_hi, float w,
                                float sample_max_value, void* workspace, size_t workspace_bytes, void* stream) {
  DSG_CHECK_ARG(sample && eps && s && workspace, "dsg_dynthresh_scale: NULL pointer");
  DSG_CHECK_ARG(n > 0 && n <= 65535, "dsg_dynthresh_scale: n=%d outside [1, 65535]", n);
  DSG_CHECK_ARG(per_sample > 0 && per_sample <= 0x7fffffff, "dsg_dynthresh_scale: per_sample=%lld outside [1, 2^31 - 1]",
                (long long)per_sample);
  DSG_CHECK_ARG(k_lo >= 0 && k_lo < per_sample && k_hi >= 0 && k_hi < per_sample,
                "dsg_dynthresh_scale: rank k_lo=%lld / k_hi=%lld outside [0, per_sample=%lld)", (long long)k_lo, (long long)k_hi,
                (long long)per_sample);
  DSG_CHECK_ARG(k_hi == k_lo || k_hi == k_lo + 1, "dsg_dynthresh_scale: rank k_hi=%lld is neither k_lo=%lld nor k_lo + 1",
                (long long)k_hi, (long long)k_lo);
  DSG_CHECK_ARG(w >= 0.f && w < 1.f, "dsg_dynthresh_scale: interpolation weight w=%g outside [0, 1)", (double)w);
  DSG_CHECK_ARG(sample_max_value >= 1.f, "dsg_dynthresh_scale: sample_max_value=%g below 1", (double)sample_max_value);
  const size_t need = (size_t)n * dsg::THR_WORDS * sizeof(uint32_t);
  if (workspace_bytes < need)
    return dsg::fail(DSG_ERR_WORKSPACE_TOO_SMALL, "dsg_dynthresh_scale: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  DSG_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "dsg_dynthresh_scale: workspace is not 4-byte aligned");
  const uint64_t in_bytes = (uint64_t)n * (uint64_t)per_sample * sizeof(float), s_bytes = (uint64_t)n * sizeof(float);
  const void* ins[2] = {sample, eps};
  for (int i = 0; i < 2; ++i) {
    DSG_CHECK_ARG(!dsg::overlaps2(s, s_bytes, ins[i], in_bytes), "dsg_dynthresh_scale: s overlaps an input (input %d)", i);
    DSG_CHECK_ARG(!dsg::overlaps2(workspace, need, ins[i], in_bytes), "dsg_dynthresh_scale: the workspace overlaps an input (input %d)", i);
  }
  DSG_CHECK_ARG(!dsg::overlaps2(workspace, need, s, s_bytes), "dsg_dynthresh_scale: the workspace overlaps s");
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  DSG_HIP(dsg::zero_words(ws, (size_t)n * dsg::THR_WORDS, st));
  // dwordx4 loads need every sample's first element on a 16-byte boundary
  const bool vec = (per_sample & 3) == 0 && dsg::aligned16(sample) && dsg::aligned16(eps);
  const uint32_t lo = (uint32_t)k_lo, hi = (uint32_t)k_hi;
  dsg::thr_pass<1>(sample, eps, ws, s, n, per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, lo, hi, w, sample_max_value, vec, st);
  dsg::thr_pass<2>(sample, eps, ws, s, n, per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, lo, hi, w, sample_max_value, vec, st);
  dsg::thr_pass<3>(sample, eps, ws, s, n, per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, lo, hi, w, sample_max_value, vec, st);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
static int thr_step_check(const char* who, const float* sample, const float* eps, const float* thr, const float* prev,
                          int64_t numel, int64_t per) {
  if (!(sample && eps && thr && prev)) return fail(DSG_ERR_INVALID_ARG, "%s: NULL pointer", who);
  if (numel <= 0) return fail(DSG_ERR_INVALID_ARG, "%s: numel must be positive", who);
  if (per <= 0 || numel % per != 0)
    return fail(DSG_ERR_INVALID_ARG, "%s: per_sample=%lld does not divide numel=%lld", who, (long long)per, (long long)numel);
  if (overlaps2(prev, (uint64_t)numel * sizeof(float), thr, (uint64_t)(numel / per) * sizeof(float)))
    return fail(DSG_ERR_INVALID_ARG, "%s: prev overlaps thr", who);
  return DSG_OK;
}
}  // namespace dsg

DSG_API int dsg_ddpm_step_thr(const float* sample, const float* eps, const float* noise, const float* thr, float* prev,
                              int64_t numel, int64_t per_sample, float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float coef_x0,
                              float coef_xt, float sigma, void* stream) {
  const int rc = dsg::thr_step_check("dsg_ddpm_step_thr", sample, eps, thr, prev, numel, per_sample);
  if (rc != DSG_OK) return rc;
  const bool vec = dsg::aligned16(sample) && dsg::aligned16(eps) && dsg::aligned16(noise) && dsg::aligned16(prev);
  const dim3 grid(dsg::philox_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((dsg::thr_step_kernel<0, true>), grid, block, 0, st, sample, eps, noise, thr, prev, numel, per_sample,
                       sqrt_beta_prod_t, sqrt_alpha_prod_t, coef_x0, coef_xt, sigma);
  else
    hipLaunchKernelGGL((dsg::thr_step_kernel<0, false>), grid, block, 0, st, sample, eps, noise, thr, prev, numel, per_sample,
                       sqrt_beta_prod_t, sqrt_alpha_prod_t, coef_x0, coef_xt, sigma);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_ddim_step_thr(const float* sample, const float* eps, const float* thr, float* prev, int64_t numel,
                              int64_t per_sample, float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float sqrt_alpha_prev,
                              float dir_coef, void* stream) {
  const int rc = dsg::thr_step_check("dsg_ddim_step_thr", sample, eps, thr, prev, numel, per_sample);
  if (rc != DSG_OK) return rc;
  const bool vec = dsg::aligned16(sample) && dsg::aligned16(eps) && dsg::aligned16(prev);
  const dim3 grid(dsg::philox_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((dsg::thr_step_kernel<1, true>), grid, block, 0, st, sample, eps, (const float*)nullptr, thr, prev, numel,
                       per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, sqrt_alpha_prev, dir_coef, 0.f);
  else
    hipLaunchKernelGGL((dsg::thr_step_kernel<1, false>), grid, block, 0, st, sample, eps, (const float*)nullptr, thr, prev, numel,
                       per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, sqrt_alpha_prev, dir_coef, 0.f);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_repaint_step(const dsg_repaint_step_args* a, void* stream) {
  DSG_CHECK_ARG(a, "dsg_repaint_step: NULL args");
  DSG_CHECK_ARG(a->sample && a->eps && a->original && a->mask && a->prev, "dsg_repaint_step: NULL pointer");
  DSG_CHECK_ARG(a->n > 0 && a->c > 0 && a->h > 0 && a->w > 0, "dsg_repaint_step: extents must be positive (n=%d c=%d h=%d w=%d)",
                a->n, a->c, a->h, a->w);
  DSG_CHECK_ARG(a->original_n == 1 || a->original_n == a->n,
                "dsg_repaint_step: original_n=%d is neither 1 nor the batch %d", a->original_n, a->n);
  DSG_CHECK_ARG(a->mask_n == 1 || a->mask_n == a->n, "dsg_repaint_step: mask_n=%d is neither 1 nor the batch %d", a->mask_n,
                a->n);
  DSG_CHECK_ARG(a->mask_c == 1 || a->mask_c == a->c, "dsg_repaint_step: mask_c=%d is neither 1 nor the channel count %d",
                a->mask_c, a->c);
  dsg::repaint_geom g;
  g.hw = (int64_t)a->h * a->w;
  g.chw = g.hw * a->c;
  g.numel = g.chw * a->n;
  g.orig_sn = a->original_n == 1 ? 0 : g.chw;
  g.m_sc = a->mask_c == 1 ? 0 : g.hw;
  g.m_sn = a->mask_n == 1 ? 0 : g.hw * a->mask_c;
  const bool vec = (g.hw & 3) == 0 && dsg::aligned16(a->sample) && dsg::aligned16(a->eps) && dsg::aligned16(a->original) &&
                   dsg::aligned16(a->mask) && dsg::aligned16(a->prev) && dsg::aligned16(a->noise) &&
                   dsg::aligned16(a->noise_out);
  const dim3 grid(dsg::philox_blocks(g.numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t s0 = (uint32_t)a->seed, s1 = (uint32_t)(a->seed >> 32), o0 = (uint32_t)a->offset, o1 = (uint32_t)(a->offset >> 32);
#define DSG_REPAINT_LAUNCH(SRC, VEC)                                                                                          \
  hipLaunchKernelGGL((dsg::repaint_step_kernel<SRC, VEC>), grid, block, 0, st, a->sample, a->eps, a->original, a->mask,       \
                     a->noise, a->prev, a->noise_out, g, a->sqrt_beta_prod_t, a->sqrt_alpha_prod_t, a->clip,                  \
                     a->sqrt_alpha_prev, a->dir_coef, a->std, a->sqrt_beta_prev, a->add_std, s0, s1, o0, o1)
  if (a->noise) {
    if (vec) DSG_REPAINT_LAUNCH(0, true); else DSG_REPAINT_LAUNCH(0, false);
  } else {
    if (vec) DSG_REPAINT_LAUNCH(1, true); else DSG_REPAINT_LAUNCH(1, false);
  }
#undef DSG_REPAINT_LAUNCH
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_repaint_undo(const float* sample, const float* noise, float* out, int64_t numel, float ck, float cz,
                             uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(sample && out, "dsg_repaint_undo: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_repaint_undo: numel must be positive");
  const bool vec = (numel & 3) == 0 && dsg::aligned16(sample) && dsg::aligned16(out) && dsg::aligned16(noise);
  const dim3 grid(dsg::philox_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t s0 = (uint32_t)seed, s1 = (uint32_t)(seed >> 32), o0 = (uint32_t)offset, o1 = (uint32_t)(offset >> 32);
#define DSG_UNDO_LAUNCH(SRC, VEC)                                                                                     \
  hipLaunchKernelGGL((dsg::repaint_undo_kernel<SRC, VEC>), grid, block, 0, st, sample, noise, out, numel, ck, cz, s0, \
                     s1, o0, o1)
  if (noise) {
    if (vec) DSG_UNDO_LAUNCH(0, true); else DSG_UNDO_LAUNCH(0, false);
  } else {
    if (vec) DSG_UNDO_LAUNCH(1, true); else DSG_UNDO_LAUNCH(1, false);
  }
#undef DSG_UNDO_LAUNCH
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
// do [a, a + bytes) and [b, b + bytes) share a byte?  (NULL overlaps nothing)
static inline bool overlaps(const void* a, const void* b, uint64_t bytes) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y ? y - x < bytes : x - y < bytes;
}

template <int ORDER, int NOISE>
static void dpmsolver_launch(const dsg_dpmsolver_step_args* a, bool vec, const float* nz, hipStream_t st) {
  const dpm_coef k = {a->sigma_s, a->alpha_s, a->inv_r0, a->inv_r1, a->q, a->p, a->kx, a->c0, a->c1, a->c2, a->cn};
  const dim3 grid(philox_blocks(a->numel)), block(256);
  const uint32_t s0 = (uint32_t)a->seed, s1 = (uint32_t)(a->seed >> 32), o0 = (uint32_t)a->offset, o1 = (uint32_t)(a->offset >> 32);
  if (vec)
    hipLaunchKernelGGL((dpmsolver_step_kernel<ORDER, NOISE, true>), grid, block, 0, st, a->sample, a->eps, a->m1, a->m2, nz,
                       a->prev, a->m0_out, a->noise_out, a->numel, k, s0, s1, o0, o1);
  else
    hipLaunchKernelGGL((dpmsolver_step_kernel<ORDER, NOISE, false>), grid, block, 0, st, a->sample, a->eps, a->m1, a->m2, nz,
                       a->prev, a->m0_out, a->noise_out, a->numel, k, s0, s1, o0, o1);
}

template <int ORDER>
static void dpmsolver_launch_order(const dsg_dpmsolver_step_args* a, bool vec, hipStream_t st) {
  if (!a->add_noise) dpmsolver_launch<ORDER, 0>(a, vec, nullptr, st);
  else if (a->noise) dpmsolver_launch<ORDER, 1>(a, vec, a->noise, st);
  else dpmsolver_launch<ORDER, 2>(a, vec, nullptr, st);
}
}  // namespace dsg

DSG_API int dsg_dpmsolver_step(const dsg_dpmsolver_step_args* a, void* stream) {
  DSG_CHECK_ARG(a, "dsg_dpmsolver_step: NULL args");
  DSG_CHECK_ARG(a->sample && a->eps && a->prev && a->m0_out, "dsg_dpmsolver_step: NULL pointer");
  DSG_CHECK_ARG(a->numel > 0, "dsg_dpmsolver_step: numel must be positive");
  DSG_CHECK_ARG(a->order >= 1 && a->order <= 3, "dsg_dpmsolver_step: order=%d is not 1, 2 or 3", a->order);
  DSG_CHECK_ARG(a->order < 2 || a->m1, "dsg_dpmsolver_step: order %d needs the history entry m1", a->order);
  DSG_CHECK_ARG(a->order < 3 || a->m2, "dsg_dpmsolver_step: order %d needs the history entry m2", a->order);
  // what THIS call reads and writes (a history entry above the order, or a noise pointer without add_noise, is not touched)
  const float* m1 = a->order >= 2 ? a->m1 : nullptr;
  const float* m2 = a->order >= 3 ? a->m2 : nullptr;
  const float* nz = a->add_noise ? a->noise : nullptr;
  float* nout = a->add_noise ? a->noise_out : nullptr;
  const uint64_t bytes = (uint64_t)a->numel * sizeof(float);
  const void* ins[5] = {a->sample, a->eps, m1, m2, nz};
  const void* outs[3] = {a->prev, a->m0_out, nout};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 5; ++i)
      DSG_CHECK_ARG(!dsg::overlaps(outs[o], ins[i], bytes), "dsg_dpmsolver_step: an output overlaps an input (output %d, input %d)",
                    o, i);
    for (int p = o + 1; p < 3; ++p)
      DSG_CHECK_ARG(!dsg::overlaps(outs[o], outs[p], bytes), "dsg_dpmsolver_step: two outputs overlap (%d, %d)", o, p);
  }
  const bool vec = dsg::aligned16(a->sample) && dsg::aligned16(a->eps) && dsg::aligned16(m1) && dsg::aligned16(m2) &&
                   dsg::aligned16(nz) && dsg::aligned16(a->prev) && dsg::aligned16(a->m0_out) && dsg::aligned16(nout);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dsg_dpmsolver_step_args b = *a;     // the kernels get exactly the pointers checked above
  b.m1 = m1; b.m2 = m2; b.noise = nz; b.noise_out = nout;
  if (a->order == 1) dsg::dpmsolver_launch_order<1>(&b, vec, st);
  else if (a->order == 2) dsg::dpmsolver_launch_order<2>(&b, vec, st);
  else dsg::dpmsolver_launch_order<3>(&b, vec, st);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

// The DEVICE address of a pinned host buffer (hipHostMalloc'ed or hipHostRegister'ed): what a kernel that reads the buffer in
// place must be given.  With torch's default pinned allocator the two addresses are equal (unified addressing); under its
// host-register configuration they need not be -- nothing here assumes it.  Fails (DSG_ERR_INVALID_ARG) for pageable memory.
DSG_API int dsg_host_device_pointer(const void* host, void** device) {
  DSG_CHECK_ARG(host && device, "dsg_host_device_pointer: NULL pointer");
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, const_cast<void*>(host), 0) != hipSuccess || d == nullptr) {
    (void)hipGetLastError();
    return dsg::fail(DSG_ERR_INVALID_ARG, "dsg_host_device_pointer: %p is not device-accessible pinned host memory", host);
  }
  *device = d;
  return DSG_OK;
}
