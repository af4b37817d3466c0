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
}  // namespace dsg

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
